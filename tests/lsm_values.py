"""The log-softmax kernels across the logit VALUE range: input profiles, the fp64 reference, the error bound and a numpy
model of the kernels' arithmetic.  A helper module (like joint_reference.py), shared by test_host_lsm_values.py,
test_gpu_lsm_values.py and tools/lsm_value_range.py.

Profiles.  Each is a function of a seeded fp32 base z = 3 * randn(rows, V) on the CPU, cast to the dtype under test
afterwards.  The fp64 reference is computed from the CAST values upcast to fp64, so the quantisation of the input is never
counted as error.

    plain                               z
    shift+100, shift-1000, shift+60000  z + c    (fp16 / bf16: a few distinct values per row at 60000 -- intended)
    spread10, spread300                 z * 10, z * 300: peaked rows, log-probs down to about -4000, sum(exp) exactly 1
                                        in most rows
    ties                                every entry of a row equal, rows alternating between 0 and 60000: -ln V everywhere
    masked                              about 30 % of each row -inf; never column 0 (the blank), never a column of
                                        ``keep`` (the labels of the utterance on the fused path); with ``single`` one row
                                        keeps ONE finite entry (plain log-softmax only: exactly 0 there, -inf elsewhere)

Out of scope, untested and not promised: rows without a finite entry, +inf, NaN, and |x| above 65504 (the largest finite
fp16; above about 2.3e38 the kernels' rounded -max * log2(e) overflows).

Bound.  For element j of a row with fp64 reference lp, row maximum mx and eps = 2^-24

    tol_j = 4 eps (|x_j - mx| + |lp_j|) + 2e-6 max(1, ln V)

The second term is the tolerance test_gpu_parity.test_log_softmax_kernel has always had; the first covers the two roundings
of the final subtractions (x_j - mx) - ls, times two.  The bound does NOT grow with |mx|: a log-softmax is invariant to a
shift of its row and so must its error be.  -inf sits exactly where the reference has it; everything else is finite.

Gradient bound.  For d/d logits of a row with gradient pair (gB, gL) on (blank, label) and upstream scale go the reference
is go (gB [j = blank] + gL [j = label] - p_j (gB + gL)) with p = softmax in fp64, and

    gtol_j = go (|gB + gL| p_j tol_j + 4 eps (|gB| + |gL|))

-- to first order a relative error in p_j is the absolute error in lp_j; the second term is the roundings of the two
products, their sum and the final add.  At masked entries the gradient is exactly 0.

Emulation.  emulate_log_softmax / emulate_backward are the kernels' arithmetic in numpy: fp32 storage, the fma with one
rounding, exact exp2 and log.  ``corrected=False`` is the arithmetic before the per-row correction (the exponent's offset
mb = -mx * log2(e) rounded to fp32 and its rounding left in log(sum); the backward through mb2 = -(mx + ls) * log2(e)),
``corrected=True`` the one the kernels have: ls += lo * ln 2 with lo = fma(-mx, log2(e), -mb), the exact residual of the
rounded product, and the backward as -e_j * (gs / s) with the forward's e_j."""
import numpy as np
import torch

EPS = 2.0 ** -24
LOG2E = np.float32(1.44269504088896340736)
LN2 = np.float32(0.69314718055994530942)
PROFILES = ("plain", "shift+100", "shift-1000", "shift+60000", "spread10", "spread300", "ties", "masked")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MASKED_FRACTION = 0.3


def base(rows, V, seed):
    """The seeded fp32 base z = 3 * randn(rows, V) (CPU)."""
    g = torch.Generator().manual_seed(int(seed))
    return 3.0 * torch.randn(rows, V, generator=g, dtype=torch.float32)


def single_finite(rows, V):
    """(row, column) of the one finite entry the masked profile leaves with ``single=True``."""
    return rows // 2, V // 3


def profile(name, z, dtype=torch.float32, keep=(), single=False):
    """Profile ``name`` of the base ``z`` (rows, V), cast to ``dtype``.  keep: columns the masked profile leaves alone
    besides column 0; single: the masked profile leaves one row with a single finite entry."""
    rows, V = z.shape
    if name == "plain":
        x = z.clone()
    elif name.startswith("shift"):
        x = z + float(name[5:])
    elif name.startswith("spread"):
        x = z * float(name[6:])
    elif name == "ties":
        x = torch.zeros_like(z)
        x[1::2] = 60000.0
    elif name == "masked":
        g = torch.Generator().manual_seed(rows * 100003 + V)
        mask = torch.rand(rows, V, generator=g) < MASKED_FRACTION
        mask[:, 0] = False
        for c in keep:
            mask[:, int(c)] = False
        x = z.masked_fill(mask, float("-inf"))
        if single:
            r, c = single_finite(rows, V)
            v = z[r, c].item()
            x[r] = float("-inf")
            x[r, c] = v
    else:
        raise ValueError(name)
    return x.to(dtype)


def reference(x):
    """fp64 log-probs (numpy) of the values of ``x`` (a tensor of any dtype, or an array), shape kept."""
    x64 = x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)
    mx = x64.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        d = x64 - mx
        return x64, d - np.log(np.exp(d).sum(-1, keepdims=True))


def tolerance(x64, lp64):
    """tol_j of the module docstring; +inf where the reference is -inf."""
    V = x64.shape[-1]
    mx = x64.max(-1, keepdims=True)
    return 4 * EPS * (np.abs(x64 - mx) + np.abs(lp64)) + 2e-6 * max(1.0, float(np.log(V)))


def log_prob_ratio(got, x64, lp64):
    """Worst error / bound of log-probs ``got`` (array or tensor).  Raises AssertionError when -inf does not sit exactly
    where the reference has it, or anything else is not finite."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    got = got.reshape(lp64.shape)
    minf = np.isneginf(lp64)
    assert np.array_equal(np.isneginf(got), minf), "-inf pattern differs from the reference's"
    fin = ~minf
    assert np.isfinite(got[fin]).all(), "non-finite log-prob where the reference is finite"
    return float((np.abs(got[fin] - lp64[fin]) / tolerance(x64, lp64)[fin]).max())


def pair_gradients(rows, seed):
    """Synthetic per-cell gradient pairs and upstream scale: gB, gL ~ U(-1, 1) (rows,), go ~ U(0.5, 1.5) scalar."""
    rng = np.random.RandomState(int(seed))
    gB = rng.uniform(-1, 1, rows).astype(np.float32)
    gL = rng.uniform(-1, 1, rows).astype(np.float32)
    return gB, gL, np.float32(rng.uniform(0.5, 1.5))


def to_diagonal(pairs):
    """(N, T, U, 2) row-major pairs in the diagonal-major layout the fused backward reads: cell (t, u) of an utterance
    sits in row (t + u) mod T."""
    N, T, U, _ = pairs.shape
    out = np.empty_like(pairs)
    t, u = np.meshgrid(np.arange(T), np.arange(U), indexing="ij")
    out[:, (t + u) % T, u] = pairs[:, t, u]
    return out


def cell_labels(labels, T, U, blank=0):
    """(T*U,) label column of every cell of ONE utterance's lattice: labels[u] for u < U - 1, the blank in the last
    column (streaming.h: map_cell)."""
    col = np.concatenate([np.asarray(labels, np.int64).reshape(-1)[:U - 1], [blank]])
    return np.tile(col, T)


def gradient_reference(x64, lp64, gB, gL, go, lab, blank=0):
    """(ref, bound) of d/d logits, fp64, (rows, V)."""
    rows, V = x64.shape
    gB64, gL64 = gB.astype(np.float64)[:, None], gL.astype(np.float64)[:, None]
    p = np.exp(lp64)
    onehot = np.zeros((rows, V))
    onehot[:, blank] += gB64[:, 0]
    np.add.at(onehot, (np.arange(rows), lab), gL64[:, 0])
    ref = float(go) * (onehot - p * (gB64 + gL64))
    tol = np.where(np.isneginf(lp64), 0.0, tolerance(x64, np.where(np.isneginf(lp64), 0.0, lp64)))
    bound = float(go) * (np.abs(gB64 + gL64) * p * tol + 4 * EPS * (np.abs(gB64) + np.abs(gL64)))
    return ref, bound


def gradient_ratio(got, ref, bound, lp64):
    """Worst error / bound of d/d logits ``got``; masked entries (reference log-prob -inf) must be exactly 0."""
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    got = got.reshape(ref.shape)
    minf = np.isneginf(lp64)
    assert (got[minf] == 0).all(), "non-zero gradient at a masked entry"
    assert np.isfinite(got).all(), "non-finite gradient"
    return float((np.abs(got - ref) / bound)[~minf].max())


# ---- the kernels' arithmetic in numpy ----
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _row_stats(x32, corrected):
    """mx, mb, e = exp2(fma(x, log2e, mb)), s = sum(e), ls (the corrected one or not) -- fp32 storage, fp64 in between."""
    x = np.asarray(x32, np.float32)
    mx = x.max(-1, keepdims=True)
    prod = -mx.astype(np.float64) * np.float64(LOG2E)          # (24 x 24 bits: exact in fp64)
    mb = _f32(prod)
    with np.errstate(over="ignore"):
        e = _f32(np.exp2(_f32(x.astype(np.float64) * np.float64(LOG2E) + mb.astype(np.float64)).astype(np.float64)))
    s = e.sum(-1, keepdims=True, dtype=np.float32)
    ls = _f32(np.log(s.astype(np.float64)))
    if corrected:
        lo = _f32(prod - mb.astype(np.float64))                # fma(-mx, log2e, -mb): exact
        ls = _f32(ls.astype(np.float64) + lo.astype(np.float64) * np.float64(LN2))
    return x, mx, mb, e, s, ls


def emulate_log_softmax(x32, corrected):
    x, mx, _, _, _, ls = _row_stats(x32, corrected)
    with np.errstate(invalid="ignore"):
        return (x - mx) - ls


def emulate_backward(x32, gB, gL, go, lab, corrected, blank=0):
    """d/d logits of the fused backward bodies (fp32, (rows, V))."""
    x, mx, _, e, s, ls = _row_stats(x32, corrected)
    rows = x.shape[0]
    go = np.float32(go)
    b, l = (gB * go).astype(np.float32)[:, None], (gL * go).astype(np.float32)[:, None]
    gs = b + l
    if corrected:
        d = -e * (gs / s)
    else:
        mb2 = _f32(-(mx + ls).astype(np.float64) * np.float64(LOG2E))
        d = -_f32(np.exp2(_f32(x.astype(np.float64) * np.float64(LOG2E) + mb2.astype(np.float64)).astype(np.float64))) * gs
    d = d.astype(np.float32)
    d[:, blank] += b[:, 0]
    np.add.at(d, (np.arange(rows), lab), l[:, 0])
    return d
