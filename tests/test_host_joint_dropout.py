"""Dropout inside the fused joint, without a GPU: the mask's definition (a NumPy restatement against the Random123 known
answers, the library's host entry against the restatement, its keep rate), the C entries of
include/warp_rnnt_amd_joint_dropout.h (their twins' argument lists with p and the seed behind them, refusing bad arguments
before any HIP call) and the device-free parts of the Python front end."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from joint_dropout_mask import keep_mask, philox4x32_10, scale, seed_u64, threshold

ENTRIES = {"rnnt_amd_joint_loss_dropout", "rnnt_amd_joint_backward_dropout", "rnnt_amd_joint_dropout_mask_host"}
INVALID, SUCCESS = 5, 0
SEEDS = (1234, -7, 2 ** 40 + 3)
PS = (0.2, 0.5, 0.9, 1e-10)


def _lib():
    import warp_rnnt_amd
    from warp_rnnt_amd import _build
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    return warp_rnnt_amd.load()


def _host_mask(seed, p, N, T, U, H):
    keep = np.full((N, T, U, H), 255, dtype=np.uint8)
    status = _lib().rnnt_amd_joint_dropout_mask_host(seed_u64(seed), p, N, T, U, H, keep.ctypes.data)
    assert status == SUCCESS
    return keep


# ---- the definition ----

@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_numpy_philox_gives_the_random123_known_answers(counter, key, want):
    assert " ".join("%08x" % int(w) for w in philox4x32_10(counter, key)) == want


def test_threshold_and_scale_of_the_fp32_probability():
    assert threshold(0.2) == 3435973824           # 0.2f is 0.20000000298...: not floor(0.8 * 2^32) = 3435973836
    assert threshold(0.5) == 2147483648
    assert threshold(0.9) == 429496832
    assert threshold(1e-10) == 2 ** 32 - 1
    assert threshold(0.0) == 2 ** 32 - 1
    assert scale(0.5) == 2.0 and scale(0.2) == float(np.float32(1.0 / (1.0 - float(np.float32(0.2)))))


def test_mask_anchor():
    """seed 1234, p = 0.5, one cell of H = 32: element 0 first, packed MSB-first."""
    bits = keep_mask(1234, 0.5, 1, 1, 1, 32).reshape(-1)
    assert "%08x" % int("".join(str(int(b)) for b in bits), 2) == "a4b53212"
    host = _host_mask(1234, 0.5, 1, 1, 1, 32).reshape(-1)
    assert "%08x" % int("".join(str(int(b)) for b in host), 2) == "a4b53212"


@pytest.mark.parametrize("shape", [(2, 5, 3, 32), (1, 1, 1, 1024)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("seed", SEEDS)
def test_host_entry_equals_the_numpy_mask(shape, seed):
    for p in PS:
        host = _host_mask(seed, p, *shape)
        assert set(np.unique(host)) <= {0, 1}                       # every byte written, as 0 or 1
        assert np.array_equal(host.astype(bool), keep_mask(seed, p, *shape)), (seed, p)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", PS[:3])
def test_keep_rate_within_four_sigma(seed, p):
    shape = (2, 16, 8, 1024)
    n = int(np.prod(shape))
    assert n == 262144
    q = threshold(p) / 2 ** 32
    bound = 4 * math.sqrt(q * (1 - q) / n)
    for mask in (keep_mask(seed, p, *shape), _host_mask(seed, p, *shape)):
        assert abs(float(mask.sum()) / n - q) <= bound, (seed, p, float(mask.sum()) / n, q, bound)


def test_mask_of_an_utterance_does_not_depend_on_the_padded_shape():
    small = _host_mask(99, 0.3, 2, 3, 2, 64)
    padded = _host_mask(99, 0.3, 3, 6, 4, 64)
    assert np.array_equal(small, padded[:2, :3, :2])


# ---- the C entries ----

def test_dropout_entries_take_the_arguments_of_their_twins_and_philox_is_one_definition_in_the_build():
    """(What every additive header owes -- declared, bound, exported, a stale library refused: test_host_additive_abi.py.)"""
    from warp_rnnt_amd import _build, _lib as lib
    assert set(lib.DROPOUT_SYMBOLS) == ENTRIES
    # the arguments of the twin with (float p, const uint64_t *seed) behind them
    for name, twin in (("rnnt_amd_joint_loss_dropout", "rnnt_amd_joint_loss"),
                       ("rnnt_amd_joint_backward_dropout", "rnnt_amd_joint_backward")):
        assert lib.DROPOUT_SYMBOLS[name][1] == lib.SYMBOLS[twin][1] + [ctypes.c_float, ctypes.c_void_p]
    # philox.h is part of the build's fingerprint
    assert "philox.h" in _build.HEADERS
    philox = open(os.path.join(_build.CSRC, "philox.h")).read()
    for const in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):
        assert const in philox
    assert not re.search(r"\basm\b", philox)


def test_dropout_entries_refuse_before_any_hip_call():
    """Dummy device pointers that are never dereferenced: each call is refused by the host-side check it names, or is one
    of the twin's answers without a launch."""
    L = _lib()
    p = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(256 + 4)

    def fwd(entry="drop", ws=p, dtype=0, act=0, f=p, g=p, w=p, labels=p, xn=p, yn=p, costs=p, lse=p, grads=p,
            N=2, T=3, U=2, H=64, V=5, blank=0, drop=0.25, seed=p):
        args = (None, ws, dtype, act, f, g, w, p, labels, xn, yn, costs, lse, grads, N, T, U, H, V, blank, 0.0)
        return L.rnnt_amd_joint_loss(*args) if entry == "twin" else L.rnnt_amd_joint_loss_dropout(*args, drop, seed)

    def bwd(entry="drop", ws=p, dtype=0, act=0, f=p, g=p, w=p, labels=p, xn=p, yn=p, costs=p, lse=p, grads=p,
            N=2, T=3, U=2, H=64, V=5, blank=0, drop=0.25, seed=p):
        args = (None, ws, dtype, act, f, g, w, p, labels, xn, yn, lse, grads, p, p, p, p, p, N, T, U, H, V, blank)
        return (L.rnnt_amd_joint_backward(*args) if entry == "twin"
                else L.rnnt_amd_joint_backward_dropout(*args, drop, seed))

    for call in (fwd, bwd):
        # p itself and its seed -- whatever else is asked, an early success included
        for bad in (-0.1, 1.0, 1.5, math.nan, math.inf, -math.inf):
            assert call(drop=bad) == INVALID and call(drop=bad, N=0) == INVALID, (call.__name__, bad)
        for seed in (None, odd, ctypes.c_void_p(256 + 1)):
            assert call(seed=seed) == INVALID and call(seed=seed, N=0) == INVALID, (call.__name__, seed)
            assert call(seed=seed, drop=0.0, N=0) == SUCCESS            # p == 0: the seed is ignored
        # every refusal of the twin, one at a time, with dropout on and with p == 0 (which is the twin)
        for kw in (dict(ws=None), dict(f=None), dict(g=None), dict(w=None), dict(xn=None), dict(yn=None),
                   dict(labels=None), dict(ws=odd), dict(f=odd), dict(w=odd), dict(lse=None),
                   dict(dtype=-1), dict(dtype=3), dict(act=2), dict(act=-1),
                   dict(H=48), dict(H=16), dict(H=1056), dict(H=0),
                   dict(V=1), dict(V=0), dict(blank=5), dict(blank=-1),
                   dict(N=-1), dict(N=70000), dict(T=0), dict(U=0), dict(T=1 << 15, U=1 << 14)):
            assert call("twin", **kw) == INVALID, (call.__name__, kw)
            assert call(**kw) == INVALID and call(drop=0.0, **kw) == INVALID, (call.__name__, kw)
            assert call(drop=0.0, seed=None, **kw) == INVALID, (call.__name__, kw)
        assert call("twin", N=0) == SUCCESS
        for drop in (0.0, 0.25, 0.999):
            assert call(N=0, drop=drop) == SUCCESS
    assert fwd("twin", costs=None) == INVALID and fwd(costs=None) == INVALID and fwd(costs=None, drop=0.0) == INVALID
    assert bwd("twin", grads=None) == INVALID and bwd(grads=None) == INVALID and bwd(grads=None, drop=0.0) == INVALID
    # the host mask: p outside [0,1), a negative size, no output
    keep = (ctypes.c_ubyte * 64)()
    assert L.rnnt_amd_joint_dropout_mask_host(1, 0.5, 1, 1, 1, 64, keep) == SUCCESS
    for bad in (-0.1, 1.0, math.nan):
        assert L.rnnt_amd_joint_dropout_mask_host(1, bad, 1, 1, 1, 64, keep) == INVALID
    assert L.rnnt_amd_joint_dropout_mask_host(1, 0.5, -1, 1, 1, 64, keep) == INVALID
    assert L.rnnt_amd_joint_dropout_mask_host(1, 0.5, 1, 1, 1, 64, None) == INVALID


# ---- the Python front end ----

def _args(N=2, T=5, U=3, H=64, V=11):
    return [torch.zeros(N, T, H), torch.zeros(N, U + 1, H), torch.zeros(V, H), torch.zeros(V),
            torch.ones(N, U, dtype=torch.int32), torch.full((N,), T, dtype=torch.int32),
            torch.full((N,), U, dtype=torch.int32)]


@pytest.mark.parametrize("bad", [1.0, -0.1, math.nan, 1.5])
def test_dropout_outside_the_unit_interval_is_a_value_error_before_every_other_check(bad):
    from warp_rnnt_amd.joint import JointLoss, rnnt_loss_from_joint
    for training in (True, False):
        with pytest.raises(ValueError, match="dropout"):
            rnnt_loss_from_joint(*_args(), dropout=bad, training=training)       # CPU tensors: before the device check
        with pytest.raises(ValueError, match="dropout"):
            rnnt_loss_from_joint(*_args(H=48), activation="gelu", dropout=bad, training=training)
    with pytest.raises(ValueError, match="dropout"):
        JointLoss(64, 11, dropout=bad)
    # a good one reaches the checks behind it
    with pytest.raises(RuntimeError, match="CUDA"):
        rnnt_loss_from_joint(*_args(), dropout=0.2)


def test_seed_resolution_is_a_pure_function():
    from warp_rnnt_amd.joint import resolve_dropout_seed
    cpu = torch.device("cpu")
    good = torch.tensor([5], dtype=torch.int64)
    assert resolve_dropout_seed(good, cpu, False) is good
    assert resolve_dropout_seed(good, cpu, True) is good                  # a given seed may be captured
    assert resolve_dropout_seed(good.reshape(()), cpu, False).numel() == 1
    with pytest.raises(RuntimeError, match="int64"):
        resolve_dropout_seed(torch.tensor([5], dtype=torch.int32), cpu, False)
    with pytest.raises(RuntimeError, match="int64"):
        resolve_dropout_seed(torch.tensor([5.0]), cpu, False)
    with pytest.raises(RuntimeError, match="one element"):
        resolve_dropout_seed(torch.tensor([5, 6], dtype=torch.int64), cpu, False)
    with pytest.raises(RuntimeError, match="one element"):
        resolve_dropout_seed(torch.zeros(0, dtype=torch.int64), cpu, False)
    with pytest.raises(RuntimeError, match="device of f"):
        resolve_dropout_seed(good, torch.device("cuda:0"), False)
    with pytest.raises(RuntimeError, match="tensor"):
        resolve_dropout_seed(5, cpu, False)
    # none given: drawn -- unless the stream is capturing
    drawn = []
    assert resolve_dropout_seed(None, cpu, False, draw=lambda d: drawn.append(d) or good) is good and drawn == [cpu]
    with pytest.raises(RuntimeError, match="explicit dropout_seed"):
        resolve_dropout_seed(None, cpu, True, draw=lambda d: drawn.append(d) or good)
    assert drawn == [cpu]
    # the default draw: int64, one element, reproduced by torch.manual_seed
    torch.manual_seed(3)
    a = resolve_dropout_seed(None, cpu, False)
    b = resolve_dropout_seed(None, cpu, False)
    torch.manual_seed(3)
    a2 = resolve_dropout_seed(None, cpu, False)
    assert a.dtype == torch.int64 and a.numel() == 1 and a.device == cpu
    assert torch.equal(a, a2) and not torch.equal(a, b)


def test_signatures():
    from warp_rnnt_amd import ops
    from warp_rnnt_amd.joint import JointLoss, rnnt_loss_from_joint
    params = list(inspect.signature(rnnt_loss_from_joint).parameters.values())
    first = [(p.name, p.default) for p in params[:12]]
    E = inspect.Parameter.empty
    assert first == [("f", E), ("g", E), ("weight", E), ("bias", E), ("labels", E), ("frames_lengths", E),
                     ("labels_lengths", E), ("activation", "tanh"), ("average_frames", False), ("reduction", "none"),
                     ("blank", 0), ("fastemit_lambda", 0.0)]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params[:12])
    rest = [(p.name, p.default, p.kind) for p in params[12:]]
    K = inspect.Parameter.KEYWORD_ONLY
    assert rest == [("dropout", 0.0, K), ("training", True, K), ("dropout_seed", None, K)]
    for fn in (ops.joint_loss, ops.joint_backward):
        tail = [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[-2:]]
        assert tail == [("dropout", 0.0), ("seed", None)], fn
    init = [(p.name, p.default) for p in list(inspect.signature(JointLoss.__init__).parameters.values())[1:]]
    assert init == [("hidden", E), ("vocab", E), ("activation", "tanh"), ("dropout", 0.0), ("bias", True), ("blank", 0),
                    ("fastemit_lambda", 0.0), ("reduction", "mean")]
    fwd = [p.name for p in list(inspect.signature(JointLoss.forward).parameters.values())[1:]]
    assert fwd == ["f", "g", "labels", "frames_lengths", "labels_lengths", "dropout_seed"]


def test_joint_loss_module_owns_linear_parameters_and_hands_its_state_on(monkeypatch):
    from warp_rnnt_amd import joint
    torch.manual_seed(0)
    m = joint.JointLoss(64, 11, activation="relu", dropout=0.2, blank=3, fastemit_lambda=0.01, reduction="sum")
    torch.manual_seed(0)
    lin = torch.nn.Linear(64, 11)
    assert isinstance(m, torch.nn.Module)
    assert torch.equal(m.weight, lin.weight) and torch.equal(m.bias, lin.bias)      # initialised as nn.Linear does
    assert [n for n, _ in m.named_parameters()] == ["weight", "bias"]
    assert joint.JointLoss(64, 11, bias=False).bias is None
    calls = []
    monkeypatch.setattr(joint, "rnnt_loss_from_joint", lambda *a, **kw: calls.append((a, kw)) or "X")
    batch = tuple(_args()[i] for i in (0, 1, 4, 5, 6))
    seed = torch.tensor([1], dtype=torch.int64)
    assert m(*batch, dropout_seed=seed) == "X"
    a, kw = calls.pop()
    assert a[0] is batch[0] and a[1] is batch[1] and a[2] is m.weight and a[3] is m.bias and a[4:] == batch[2:]
    assert kw == dict(activation="relu", reduction="sum", blank=3, fastemit_lambda=0.01, dropout=0.2, training=True,
                      dropout_seed=seed)
    m.eval()
    m(*batch)
    assert calls.pop()[1]["training"] is False
