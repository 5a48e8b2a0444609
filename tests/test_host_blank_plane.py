"""Host side of the blank plane (warp_rnnt_amd/ops.py): when log_softmax produces it, when a loss call may
take it, and what the new C entries answer without a launch.  No GPU needed."""
import pytest
import torch

from warp_rnnt_amd import _lib, ops

P = 1 << 40          # "a device pointer": non-null, aligned, never dereferenced (every call below returns before a launch)


@pytest.mark.parametrize("cells,V,want", [
    (16 * 1500 * 300, 50, True),          # c4 of bench.py
    (8 * 1500 * 300, 10000, True),        # c5
    (32 * 150 * 20, 5000, False),         # c3: 96 k cells, launch-bound
    (16 * 150 * 40, 28, False),           # c2: rows inside one line, and small
    (16 * 1500 * 300, 32, False),         # 4V = 128: blank and label share the row's line(s)
    (16 * 1500 * 300, 28, False),
    (16 * 1500 * 300, 33, True),          # the first V whose rows outgrow a line
    ((1 << 20) - 1, 50, False),
    (1 << 20, 50, True),
    (0, 50, False),
])
def test_policy_table(cells, V, want):
    assert ops.wants_blank_plane(cells, V) is want


def test_policy_is_a_function_of_the_shape_alone(monkeypatch):
    monkeypatch.setenv("RNNT_BLANK_PLANE", "0")
    assert ops.wants_blank_plane(1 << 22, 50)
    assert ops.PLANE_MIN_CELLS == 1 << 20 and ops.PLANE_COLUMN == 0


def _note(plane, t, column=0):
    return (plane, t._version, column, t.data_ptr())


def test_note_validity_predicate():
    lp = torch.zeros(2, 3, 4, 5)
    plane = torch.zeros(2 * 3 * 4)
    facts = dict(version=lp._version, data_ptr=lp.data_ptr(), shape=tuple(lp.shape), dtype=lp.dtype, contiguous=True,
                 blank=0)
    good = _note(plane, lp)
    assert ops.plane_note_valid(good, **facts)
    assert not ops.plane_note_valid(None, **facts)
    assert not ops.plane_note_valid(good[:3], **facts)
    assert not ops.plane_note_valid(good, **dict(facts, version=facts["version"] + 1))
    assert not ops.plane_note_valid(good, **dict(facts, data_ptr=facts["data_ptr"] + 4))
    assert not ops.plane_note_valid(good, **dict(facts, blank=3))
    assert not ops.plane_note_valid(good, **dict(facts, shape=(2, 3, 20)))
    assert not ops.plane_note_valid(good, **dict(facts, shape=(2, 3, 4, 5, 1)))
    assert not ops.plane_note_valid(good, **dict(facts, dtype=torch.float16))
    assert not ops.plane_note_valid(good, **dict(facts, contiguous=False))
    assert not ops.plane_note_valid(_note(torch.zeros(23), lp), **facts)
    assert not ops.plane_note_valid(_note(None, lp), **facts)


def test_the_note_lives_on_one_object_and_dies_with_its_values():
    lp = torch.zeros(2, 3, 4, 5)
    plane = torch.zeros(24)
    setattr(lp, ops.PLANE_ATTR, _note(plane, lp))
    assert ops.blank_plane_of(lp, 0) is plane
    assert ops.blank_plane_of(lp, 3) is None                   # made for column 0
    assert ops.blank_plane_of(lp.view(2, 3, 4, 5), 0) is None  # a view is another object
    assert ops.blank_plane_of(lp.clone(), 0) is None
    assert ops.blank_plane_of(lp.detach(), 0) is None
    assert ops.blank_plane_of(torch.zeros(2, 3, 4, 5), 0) is None
    lp.add_(1.0)                                               # the version counter moves
    assert ops.blank_plane_of(lp, 0) is None
    lp2 = torch.zeros(2, 3, 4, 5)
    setattr(lp2, ops.PLANE_ATTR, _note(plane, lp2))
    lp2.set_(torch.zeros(2, 3, 4, 5))                          # other storage (the version moves as well)
    assert ops.blank_plane_of(lp2, 0) is None
    lp3 = torch.zeros(2, 3, 4, 5)
    setattr(lp3, ops.PLANE_ATTR, _note(plane, lp3))
    ops._drop_plane(lp3)                                       # what every raw-pointer writer does first
    assert not hasattr(lp3, ops.PLANE_ATTR) and ops.blank_plane_of(lp3, 0) is None
    ops._drop_plane(lp3)
    ops._drop_plane(None)


def test_new_entries_are_declared_bound_and_answer_without_a_launch():
    import os
    L = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "warp_rnnt_amd.h")).read().replace(" (", "(")
    names = ("rnnt_amd_log_softmax_plane", "rnnt_amd_log_softmax_plane_typed", "rnnt_amd_loss_blank_plane",
             "rnnt_amd_debug_gather_only_blank_plane")
    for name in names:
        assert name + "(" in hdr and name in _lib.SYMBOLS
    assert L.rnnt_amd_version() == _lib.ABI_VERSION          # additive entries: the number stays
    # log-softmax with a plane: stream x out col_out rows V col
    base = dict(x=P, out=P, col_out=P, rows=4, V=7, col=0)
    for bad in (dict(rows=-1), dict(V=0), dict(col=-1), dict(col=7), dict(col_out=0)):
        a = dict(base, **bad)
        assert L.rnnt_amd_log_softmax_plane(0, a["x"], a["out"], a["col_out"], a["rows"], a["V"], a["col"]) == 5, bad
        for dtype in (0, 1, 2):
            assert L.rnnt_amd_log_softmax_plane_typed(0, dtype, a["x"], a["out"], a["col_out"], a["rows"], a["V"],
                                                      a["col"]) == 5, bad
    for dtype in (-1, 3):
        assert L.rnnt_amd_log_softmax_plane_typed(0, dtype, P, P, P, 4, 7, 0) == 5
    # the loss: stream workspace log_probs blank_plane labels xn yn costs grads grads_kind N T U V blank fastemit_lambda
    base = dict(workspace=P, log_probs=P, blank_plane=P, labels=P, xn=P, yn=P, costs=P, grads=P, grads_kind=1, N=2, T=5,
                U=3, V=7, blank=0)
    order = "workspace log_probs blank_plane labels xn yn costs grads grads_kind N T U V blank".split()

    def loss(**change):
        a = dict(base, **change)
        return L.rnnt_amd_loss_blank_plane(0, *[a[k] for k in order], 0.0)

    for bad in (dict(blank_plane=0), dict(N=-1), dict(T=0), dict(U=0), dict(N=65536), dict(workspace=0),
                dict(workspace=P + 8), dict(V=0), dict(blank=-1), dict(blank=7), dict(labels=0), dict(grads_kind=-1),
                dict(grads_kind=4), dict(grads=0)):
        assert loss(**bad) == 5, bad
    assert loss(N=0) == 0
    assert type(loss(N=0)) is int
    # the gather alone: stream workspace log_probs blank_plane labels N T U V blank
    gbase = dict(workspace=P, log_probs=P, blank_plane=P, labels=P, N=2, T=5, U=3, V=7, blank=0)
    gorder = "workspace log_probs blank_plane labels N T U V blank".split()
    for bad in (dict(blank_plane=0), dict(workspace=0), dict(N=-1), dict(T=0), dict(V=0), dict(blank=7), dict(labels=0)):
        a = dict(gbase, **bad)
        assert L.rnnt_amd_debug_gather_only_blank_plane(0, *[a[k] for k in gorder]) == 5, bad
