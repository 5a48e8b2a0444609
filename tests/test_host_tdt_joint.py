"""The joint network fused into the TDT loss without a GPU: the fp64 reference (tests/tdt_joint_reference.py) against
central differences of its own costs, the additive contract of include/warp_rnnt_amd_tdt_joint.h and its table, the
workspace size, the C entries' refusals with pointers that are never dereferenced, and the front end's argument errors."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from tdt_joint_reference import tdt_joint_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "warp_rnnt_amd_tdt_joint.h"
ENTRIES = {"rnnt_amd_tdt_joint_workspace_size", "rnnt_amd_tdt_joint_loss", "rnnt_amd_tdt_joint_backward"}
INVALID, SUCCESS = 5, 0
TDT_MAX_D = 9


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


# ---- (a) the reference's gradients against central differences of its own costs ----

@pytest.mark.parametrize("durations", [(0, 1), (1, 2)], ids=str)
def test_reference_gradients_against_central_differences(durations):
    N, T, U, V, H = 2, 4, 2, 3, 32
    D = len(durations)
    gen = torch.Generator().manual_seed(7 + durations[0])
    f = torch.randn(N, T, H, generator=gen, dtype=torch.float64) * 0.5
    g = torch.randn(N, U + 1, H, generator=gen, dtype=torch.float64) * 0.5
    w = torch.randn(V + D, H, generator=gen, dtype=torch.float64) / H ** 0.5
    b = torch.randn(V + D, generator=gen, dtype=torch.float64) * 0.1
    labels = torch.tensor([[1, 2], [2, 1]], dtype=torch.int32)
    xn, yn = torch.tensor([T, T - 1], dtype=torch.int32), torch.tensor([U, 1], dtype=torch.int32)
    weights = torch.tensor([0.5, 0.75], dtype=torch.float64)
    kw = dict(durations=durations, act="tanh", blank=0, sigma=0.05, lam=0.0)
    costs, *grads = tdt_joint_reference(f, g, w, b, labels, xn, yn, weights=weights, **kw)
    assert torch.isfinite(costs).all()

    def value(args):
        c = tdt_joint_reference(*args, labels, xn, yn, want_grads=False, **kw)[0]
        return float((c * weights).sum())

    step = 1e-5
    params = [f, g, w, b]
    for k, (x, grad) in enumerate(zip(params, grads)):
        numeric = torch.zeros_like(x)
        flat, out = x.reshape(-1), numeric.reshape(-1)
        for i in range(flat.numel()):
            keep = float(flat[i])
            flat[i] = keep + step
            up = value(params)
            flat[i] = keep - step
            down = value(params)
            flat[i] = keep
            out[i] = (up - down) / (2 * step)
        err = float((numeric - grad).abs().max() / grad.abs().max())
        print(f"durations {durations}: d/d {'fgWb'[k]} against central differences: {err:.2e} of the largest entry")
        assert err < 1e-6, ("fgWb"[k], err)


# ---- (b) the additive contract for the new header ----

def test_header_declares_what_the_table_binds_and_the_library_exports():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build, _lib as lib
    L = _lib()
    table = lib.TDT_JOINT_SYMBOLS
    assert set(table) == ENTRIES and lib.ADDITIVE_TDT_JOINT == ((table, HEADER),)
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    declared = set(re.findall(r"\b(run_[a-z_]+|rnnt_amd_[a-z_]+)\s*\(", text))
    assert declared == set(table)
    assert '#include "warp_rnnt_amd.h"' in text
    main = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    earlier = lib.ADDITIVE + lib.ADDITIVE_NEXT
    others = [lib.SYMBOLS] + [t for t, _ in earlier]
    syms = subprocess.check_output(["nm", "-D", "--defined-only", warp_rnnt_amd.lib_path()]).decode()
    for name in declared:
        assert name + "(" not in main.replace(" (", "(")                   # a header of their own
        assert not any(name in other for other in others)                 # ... and a table of their own
        assert re.search(r"\bT " + name + r"\b", syms), name
        fn = getattr(L, name)
        res, args = table[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)      # bound by load()
    for _, header in earlier:                                             # no other header declares them either
        assert not declared & set(re.findall(r"\b(rnnt_amd_[a-z_]+)\s*\(", open(os.path.join(ROOT, "include", header)).read()))
    assert L.rnnt_amd_version() == lib.ABI_VERSION == 110                 # the version did not move
    assert len(lib.ADDITIVE) == 5 and len(lib.ADDITIVE_NEXT) == 1         # ... and neither did the earlier tables
    # part of the build's fingerprint
    assert any(os.path.basename(h) == HEADER for h in _build.HEADERS)
    assert "joint_tile.h" in _build.HEADERS and "tdt_joint.h" in _build.HEADERS
    assert "tdt_joint.hip" in _build.SOURCES and "joint.hip" in _build.SOURCES
    # the argument lists: the joint entries' with the TDT loss's durations, D, sigma and the dropout's (p, seed)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    joint_fwd = lib.SYMBOLS["rnnt_amd_joint_loss"][1]
    assert table["rnnt_amd_tdt_joint_loss"][1] == joint_fwd[:11] + [vp, i] + joint_fwd[11:-1] + [f, f, f, vp]
    joint_bwd = lib.SYMBOLS["rnnt_amd_joint_backward"][1]
    assert table["rnnt_amd_tdt_joint_backward"][1] == joint_bwd[:-1] + [i, i, f, vp]
    assert table["rnnt_amd_tdt_joint_workspace_size"] == (ctypes.c_size_t, [i] * 6)


def test_library_without_an_entry_of_the_table_is_refused_with_the_rebuild_message(monkeypatch):
    from warp_rnnt_amd import _lib as lib
    _lib()
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setitem(lib.TDT_JOINT_SYMBOLS, "rnnt_amd_no_such_entry", (ctypes.c_int, [ctypes.c_float]))
    with pytest.raises(RuntimeError, match=r"rnnt_amd_no_such_entry \(include/" + re.escape(HEADER) + r"\).*rebuild it"):
        lib.load()


def test_the_units_share_one_tile_header_and_hold_no_assembly_no_atomics():
    from warp_rnnt_amd import _build
    assert "tdt_joint.hip" not in _build.HAZARD_CHECKED and "tdt_joint.hip" not in _build.RELOAD_CHECKED
    unit = open(os.path.join(_build.CSRC, "tdt_joint.hip")).read()
    joint = open(os.path.join(_build.CSRC, "joint.hip")).read()
    tile = open(os.path.join(_build.CSRC, "joint_tile.h")).read()
    for word in ("asm", "atomic", "volatile", "__syncthreads"):
        assert word not in unit, word
    assert "#pragma clang fp contract(off)" in unit
    for kernel in ("k_tdt_joint_fwd", "k_tdt_joint_bwd_fg", "k_tdt_joint_bwd_w"):
        assert kernel in unit and kernel not in joint
    # one copy of the shared pieces: defined in the header, in neither unit
    for piece in ("struct JFrag", "jf4 mma_k(", "int b_slot(", "pack_acc(const jf4", "float act_fwd(", "float act_bwd(",
                  "int hs_pitch(", "void stage_h(", "jf4 z_block(", "unsigned drop4(", "E drop_stage(", "bool dropped(",
                  "int waves_per_group(", "unsigned blocks_for(", "void k_joint_transpose_w(", "void k_joint_reduce_w("):
        assert piece in tile and piece not in unit and piece not in joint, piece
    assert '#include "joint_tile.h"' in unit and '#include "joint_tile.h"' in joint


# ---- (c) the workspace ----

def test_workspace_size():
    L = _lib()
    size, tdt_size = L.rnnt_amd_tdt_joint_workspace_size, L.rnnt_amd_tdt_workspace_size
    base = dict(N=2, T=10, U=5, H=64, V=50, D=5)

    def of(**kw):
        a = dict(base, **kw)
        return size(a["N"], a["T"], a["U"], a["H"], a["V"], a["D"])

    assert of() == of() > 0 and of() % 256 == 0
    assert of() >= tdt_size(2, 10, 5, 5)
    for shape in (dict(), dict(D=1, V=2, H=32), dict(D=9, H=1024, V=1025), dict(U=1024, T=3)):
        a = dict(base, **shape)
        assert of(**shape) % 256 == 0 and of(**shape) >= tdt_size(a["N"], a["T"], a["U"], a["D"]) > 0, shape
    for bad in ([dict(H=h) for h in (0, 16, 48, 1056)] + [dict(V=1), dict(D=0), dict(D=TDT_MAX_D + 1), dict(U=1025),
                dict(T=0), dict(N=-1)]):
        assert of(**bad) == 0, bad
    # the part beyond the TDT layout -- W^T and the split-K partials -- does not grow with the number of cells
    beyond = [of(N=n, T=100, U=20) - tdt_size(n, 100, 20, 5) for n in (8, 16)]
    assert beyond[0] == beyond[1] > 0, beyond
    assert of(N=16, T=1500, U=301, H=640, V=1025) - tdt_size(16, 1500, 301, 5) < 64 << 20
    from warp_rnnt_amd import ops
    with pytest.raises(RuntimeError, match="status 5.*unsupported sizes.*H=48"):
        ops._workspace("cpu", size, "N T U H V D", 2, 10, 5, 48, 50, 5)


# ---- (d) refusals and early successes ----

def _entries():
    L = _lib()
    p = ctypes.c_void_p(256)                 # aligned, non-null, never dereferenced
    good = (ctypes.c_int * 5)(0, 1, 2, 3, 4)

    def durs(durations):
        if isinstance(durations, (tuple, list)):
            return (ctypes.c_int * max(len(durations), 1))(*durations)
        return durations

    def fwd(ws=p, dtype=0, act=0, f=p, g=p, w=p, labels=p, xn=p, yn=p, durations=good, D=5, costs=p, stats=p, grads=p,
            N=2, T=3, U=2, H=64, V=5, blank=0, sigma=0.0, p_drop=0.0, seed=None):
        return L.rnnt_amd_tdt_joint_loss(None, ws, dtype, act, f, g, w, p, labels, xn, yn, durs(durations), D, costs,
                                         stats, grads, N, T, U, H, V, blank, sigma, 0.0, p_drop, seed)

    def bwd(ws=p, dtype=0, act=0, f=p, g=p, w=p, labels=p, xn=p, yn=p, stats=p, grads=p, D=5,
            N=2, T=3, U=2, H=64, V=5, blank=0, p_drop=0.0, seed=None):
        return L.rnnt_amd_tdt_joint_backward(None, ws, dtype, act, f, g, w, p, labels, xn, yn, stats, grads, p, p, p, p,
                                             p, N, T, U, H, V, D, blank, p_drop, seed)

    return fwd, bwd


def test_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names; what is
    not refused is an empty batch, which succeeds without a launch.  The list is tests/test_host_joint.py's, plus what the
    TDT side and the dropout add."""
    fwd, bwd = _entries()
    p = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(256 + 4)
    for call in (fwd, bwd):
        for kw in (dict(ws=None), dict(f=None), dict(g=None), dict(w=None), dict(xn=None), dict(yn=None),
                   dict(labels=None), dict(ws=odd), dict(f=odd), dict(w=odd),
                   dict(dtype=-1), dict(dtype=3), dict(act=2), dict(act=-1),
                   dict(H=48), dict(H=16), dict(H=1056), dict(H=0),
                   dict(V=1), dict(V=0), dict(blank=5), dict(blank=-1),
                   dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(T=1 << 15, U=1 << 14),
                   dict(D=0), dict(D=TDT_MAX_D + 1), dict(U=1025), dict(U=1025, T=1),
                   dict(p_drop=1.0), dict(p_drop=-0.1), dict(p_drop=float("nan")), dict(p_drop=1.5, seed=p),
                   dict(p_drop=0.3), dict(p_drop=0.3, seed=odd)):
            assert call(**kw) == INVALID, (call.__name__, kw)
            if "N" not in kw:       # a refused argument is not answered as an empty batch
                assert call(N=0, **kw) == INVALID, (call.__name__, kw)
    for durations in ((0, 1, 1), (0, 2, 3), (0, 1, 9), (-1, 0, 1), (1, 1)):        # duplicate, no 1, greater than 8
        assert fwd(durations=durations, D=len(durations)) == INVALID, durations
    assert fwd(durations=None) == INVALID
    for sigma in (-0.01, float("nan"), float("inf")):
        assert fwd(sigma=sigma) == INVALID, sigma
    assert fwd(costs=None) == INVALID
    assert fwd(stats=None) == INVALID                                # grads asked for without stats
    assert fwd(stats=ctypes.c_void_p(256 + 8)) == INVALID
    assert bwd(stats=None) == INVALID and bwd(grads=None) == INVALID
    # N == 0 is a valid empty batch: nothing to launch
    assert fwd(N=0) == SUCCESS and bwd(N=0) == SUCCESS
    assert fwd(N=0, stats=None, grads=None) == SUCCESS               # costs only
    assert fwd(N=0, p_drop=0.3, seed=p) == SUCCESS and bwd(N=0, p_drop=0.3, seed=p) == SUCCESS
    assert fwd(N=0, p_drop=0.0, seed=None, U=1, labels=None) == SUCCESS
    for durations in ((1,), (0, 1), (2, 0, 1), (1, 2), (0, 1, 8), tuple(range(9))):
        assert fwd(durations=durations, D=len(durations), N=0) == SUCCESS, durations
    for dtype in (0, 1, 2):
        assert fwd(dtype=dtype, act=1, N=0, U=1024, H=1024, sigma=0.05) == SUCCESS


# ---- (e) the front end ----

def _args(N=2, T=5, U=3, H=64, V=11, D=5, dtype=torch.float32):
    f = torch.zeros(N, T, H, dtype=dtype)
    g = torch.zeros(N, U + 1, H, dtype=dtype)
    w = torch.zeros(V + D, H)
    b = torch.zeros(V + D)
    labels = torch.ones(N, U, dtype=torch.int32)
    xn = torch.full((N,), T, dtype=torch.int32)
    yn = torch.full((N,), U, dtype=torch.int32)
    return [f, g, w, b, labels, xn, yn]


def test_front_end_signature_and_argument_errors():
    from warp_rnnt_amd import ops, tdt
    params = inspect.signature(tdt.tdt_loss_from_joint).parameters
    assert list(params) == ["f", "g", "weight", "bias", "labels", "frames_lengths", "labels_lengths", "durations", "sigma",
                            "blank", "activation", "fastemit_lambda", "average_frames", "reduction", "dropout", "training",
                            "dropout_seed"]
    assert [params[k].default for k in list(params)[7:]] == [(0, 1, 2, 3, 4), 0.0, 0, "tanh", 0.0, False, "none", 0.0,
                                                             True, None]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("dropout", "training", "dropout_seed"))
    assert hasattr(ops, "tdt_joint_loss") and hasattr(ops, "tdt_joint_backward")
    fn = tdt.tdt_loss_from_joint
    a = _args()
    a[3] = torch.zeros(11)                                  # weight rows are V + D: a bias of V entries disagrees
    with pytest.raises(RuntimeError, match="bias must be"):
        fn(*a)
    with pytest.raises(RuntimeError, match="status 5.*V \\+ D"):
        fn(*_args(V=1, D=5))                                # six rows and five durations leave one token
    with pytest.raises(RuntimeError, match="status 5.*blank"):
        fn(*_args(), blank=11)                              # a duration row
    with pytest.raises(RuntimeError, match="status 5"):
        fn(*_args(), blank=16)
    with pytest.raises(RuntimeError, match="status 5.*durations"):
        fn(*_args(D=2), durations=(0, 2))
    with pytest.raises(RuntimeError, match="status 5.*sigma"):
        fn(*_args(), sigma=-1.0)
    with pytest.raises(RuntimeError, match="status 5"):
        fn(*_args(H=48))
    with pytest.raises(RuntimeError, match="activation"):
        fn(*_args(), activation="gelu")
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="dropout"):
            fn(*_args(), dropout=bad)
    with pytest.raises(AssertionError):
        fn(*_args(), reduction="avg")
    with pytest.raises(RuntimeError, match="CUDA"):          # well-formed, but no GPU tensors
        fn(*_args())
    with pytest.raises(RuntimeError, match="CUDA"):
        fn(*_args(), dropout=0.3, training=False)


def test_module_owns_a_linear_of_vocab_plus_durations_rows():
    from warp_rnnt_amd import tdt
    torch.manual_seed(0)
    m = tdt.TDTJointLoss(64, 11, durations=[0, 1, 2], sigma=0.05, blank=10, activation="relu", dropout=0.2)
    torch.manual_seed(0)
    lin = torch.nn.Linear(64, 14)
    assert isinstance(m, torch.nn.Module) and m.weight.shape == (14, 64) and m.bias.shape == (14,)
    assert torch.equal(m.weight, lin.weight) and torch.equal(m.bias, lin.bias)       # initialised as nn.Linear does
    assert (m.durations, m.sigma, m.blank, m.activation, m.dropout, m.reduction) == ((0, 1, 2), 0.05, 10, "relu", 0.2,
                                                                                     "mean")
    assert tdt.TDTJointLoss(32, 5, bias=False).bias is None
    with pytest.raises(ValueError):
        tdt.TDTJointLoss(64, 11, dropout=1.0)
    with pytest.raises(ValueError):
        tdt.TDTJointLoss(64, 11, activation="gelu")
    for word in ("omega", "clamp", "compact layout", "U > 1024"):
        assert word in tdt.tdt_loss_from_joint.__doc__, word
    assert "joint entry" in tdt.__doc__ and "tdt_loss_from_joint" in tdt.__doc__
    hdr = open(os.path.join(ROOT, "include", "warp_rnnt_amd_tdt.h")).read()
    assert "warp_rnnt_amd_tdt_joint.h" in hdr
