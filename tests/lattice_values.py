"""The lattice sweeps and the gradient kernel across the VALUE range of their log-prob pairs: input profiles, the fp64
reference, a derived per-cell error bound and a numpy model of the sweeps' arithmetic.  A helper module (like lsm_values.py),
shared by test_host_lattice_values.py, test_gpu_lattice_values.py and tools/lattice_value_range.py; it imports no GPU code.

Profiles.  Each is a function of (seed, T, U) returning fp32 pairs (T, U, 2) in the gathered layout (channel 0 the blank,
channel 1 the label of the column; the last column's label slot holds the blank, as the gather writes it).  The base is p:
the pairs gathered from log_softmax(randn(T, U, 6)) with labels drawn in 1..5.

    plain       p                                           today's regime, the control
    spread30    the same with the logits * 30                log-probs from about 0 down to -300
    shift-100   p - 100                                      unnormalised input, |alpha| up to about 1.2e5 at T + U = 1170:
                                                             one ulp of the cost is 8e-3 there
    shift+3     p + 3                                        positive log-probs, lattices that grow upwards
    ties        every entry fp32(-ln 2)                      skip == emit at every interior cell; alpha has the closed form
                                                             log C(t+u, u) - (t+u) ln 2  (ties_alpha)
    floor-1e4   30 % of the label entries replaced by -1e4   |skip - emit| far beyond where exp2 returns 0; lattice values
                                                             down to -1e6 off the path next to values of order 100 on it
    path        every entry -60 - 20 |randn|, except along   cost 0.06 .. 1, posteriors 0 or 1, u = 1 + e rounds to 1 almost
                one seeded monotone path from (0, 0) to      everywhere
                (T-1, U-1) whose entries, and the final
                blank, are -1e-3 |randn|

Out of scope, untested here and not promised: -inf and NaN inputs (their patterns are
test_gpu_parity.test_masked_log_probs_nan_pattern_equals_the_oracles' business) and values whose running sums overflow fp32.

Reference.  `reference` computes, in fp64 and for ONE utterance of Tn x Un live cells, alphas, betas, the cost, the alpha-side
log-likelihood and the two gradient channels with FastEmit, vectorised along anti-diagonals (as
oracle.transduce_np._sweeps_fast, restated for pairs so that the bound can ride along).

Per-cell bound (derived, not measured).  Let eps = 2^-24 (half an ulp, relative).  A cell of a sweep is
    skip = v[t-1, u] + lpB      emit = v[t, u-1] + lpL      val = mx + l,  mx = max(skip, emit),  l = log1p(exp(-|skip-emit|))
(beta: the mirror image).  To first order an error d_s in skip and d_e in emit reaches val as w_s d_s + w_e d_e with the
softmax weights w_s = exp(skip - val), w_e = exp(emit - val) of the two sides (the derivative of a log-sum-exp), so with
B[.] the bound of the neighbour cells

    B[t, u] = w_s (B[t-1, u] + eps |skip|) + w_e (B[t, u-1] + eps |emit|) + eps |val| + 8 eps

The three eps |.| terms are the roundings of the two extending adds and of mx + l.  The constant covers l in [0, ln 2] as the
kernels compute it, l = fma(log2(u), ln2, e - (u - 1)) with e = exp2(-|t| log2e), u = fl(1 + e):
  * the rounding of |t| * log2e (and of the constant log2e itself, 0.22 eps relative): a relative error r in the exponent
    moves e by r |t| e and l by e / (1 + e) of that -- |t| e^-|t| <= 0.37, so 0.37 eps + 0.08 eps;
  * one ulp (2 eps relative) of the hardware exp2: 2 eps e / (1 + e) <= 1 eps;
  * the rounding of 1 + e is carried exactly by c = e - (u - 1); adding c instead of log(1 + c / u) leaves c (1 - 1/u)
    <= 0.5 eps;
  * one ulp of the hardware log2 at a value in [0.5, 1], times ln 2: 0.69 eps -- and the rounded constant ln2: 0.35 eps;
  * the rounding of the fma: half an ulp of l <= ln 2: 0.69 eps.
That is 3.7 eps; 8 eps leaves a factor of two for a libm whose expf and log1pf are good to an ulp rather than half of one
(the C oracle).  Where e underflows the error is e itself, below 2^-126.  Rim cells -- alpha[0, u], alpha[t, 0] and their
mirror images, plain sums in the reference and in the kernels -- carry their one side with weight 1 and the other with 0.
alpha[0, 0] = 0 is exact (bound 0); the last cell of beta, a copy of its blank log-prob, has eps |lpB|.
Second-order terms are of the size B^2 / 8: 1e-5 where B itself is 1e-2, the largest it gets here.

Cost: B_beta[0, 0] + eps |cost|.  Alpha-side log-likelihood alpha[Tn-1, Un-1] + lpB: B_alpha[Tn-1, Un-1] + eps |ll|.

Gradient bound.  With x = alpha + beta_next + lp - b00 in fp64 (beta_next: beta[t+1, u] for the blank channel, beta[t, u+1]
for the label channel, nothing in the last cell) and g = -exp(x), or -(1 + lambda) exp(x) for the label channel:

    E   = B_alpha[t, u] + B_beta[next cell] + B_beta[0, 0] + 4 eps (|alpha + beta_next| + |b00| + |x|)
    tol = |g| expm1(E) + 4 eps |g| + 2^-126

E bounds the error of the exponent: the three lattice values it is made of and the three roundings of its adds (the middle
one, (alpha + beta_next) + lp, is of magnitude <= |b00| + |x|); 4 eps |g| is expf to an ulp, the FastEmit product and the
conversions; 2^-126 covers a subnormal result flushed to 0.

Ratios.  lattice_ratios / gradient_ratios return (worst, rms) of |got - ref| / bound over the live cells with a positive
bound; a cell whose bound is 0 must be exact, a live value that is not finite raises, and dead cells of the gradient
(t >= Tn or u >= Un) must be exactly 0.

Emulation.  emulate_sweeps is the sweeps in fp32 numpy, diagonal-vectorised, with fp32 storage after every operation the
kernels round; it takes the log-sum-exp as an argument (lse_kernel: the kernels' step; the wrong variants of
test_host_lattice_values.py show that the bound has teeth)."""
import functools
import math

import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -126
LSE_CONSTANT = 8.0                     # the "8 eps" of the bound (test_host_lattice_values.py loosens it by hand, once)
LAMBDA = 0.01                          # FastEmit, everywhere in these tests
V = 6
PROFILES = ("plain", "spread30", "shift-100", "shift+3", "ties", "floor-1e4", "path")
# (N, T, U): each below 2^20 cells and the smallest that reaches its kernel (test_gpu_wd.test_the_launch_runs_what_the_plan_
# says and the long-sweep rows of test_gpu_wd.SHAPES)
SHAPES = ((2, 40, 33),        # wd, plain launch
          (2, 40, 130),       # wl
          (2, 130, 400),      # wd with rings
          (2, 60, 700),       # the striped single-role kernel under the ws pin
          (2, 1100, 70),      # blocks of sixteen diagonals
          (3, 1030, 129))     # long sweep, several column blocks, U - 1 on a block edge
SEED = 7
FLOOR_FRACTION = 0.3
NEG_LN2 = np.float32(-math.log(2.0))
LOG2E = np.float32(1.44269504088896340736)
LN2 = np.float32(0.693147180559945309417)


# ---- profiles ----
def _log_softmax64(z):
    m = z.max(-1, keepdims=True)
    return (z - m) - np.log(np.exp(z - m).sum(-1, keepdims=True))


def _base(rng, T, U, scale):
    """Pairs gathered from log_softmax(scale * randn(T, U, V)) (fp64 log-softmax, rounded once) with labels in 1..V-1."""
    z = rng.randn(T, U, V).astype(np.float32).astype(np.float64) * scale
    labels = rng.randint(1, V, size=(max(U - 1, 0),))
    lp = _log_softmax64(z)
    col = np.concatenate([labels, [0]]).astype(np.int64)          # the last column's label slot holds the blank
    return np.stack([lp[:, :, 0], lp[:, np.arange(U), col]], -1).astype(np.float32)


def monotone_path(rng, T, U):
    """A seeded monotone path from (0, 0) to (T-1, U-1): moves (T + U - 2,), 0 = a frame down (blank), 1 = a label right."""
    moves = np.concatenate([np.zeros(T - 1, np.int64), np.ones(U - 1, np.int64)])
    rng.shuffle(moves)
    return moves


def profile(name, seed, T, U):
    """Profile ``name``: fp32 pairs (T, U, 2)."""
    rng = np.random.RandomState(int(seed))
    if name == "plain":
        return _base(rng, T, U, 1.0)
    if name == "spread30":
        return _base(rng, T, U, 30.0)
    if name.startswith("shift"):
        return (_base(rng, T, U, 1.0) + np.float32(float(name[5:]))).astype(np.float32)
    if name == "ties":
        return np.full((T, U, 2), NEG_LN2, np.float32)
    if name == "floor-1e4":
        p = _base(rng, T, U, 1.0)
        p[..., 1][rng.rand(T, U) < FLOOR_FRACTION] = -1e4
        return p
    if name == "path":
        p = (-60.0 - 20.0 * np.abs(rng.randn(T, U, 2))).astype(np.float32)
        moves = monotone_path(rng, T, U)
        u = np.concatenate([[0], np.cumsum(moves)])
        t = np.arange(T + U - 1) - u
        on = (-1e-3 * np.abs(rng.randn(T + U - 1))).astype(np.float32)
        p[t[:-1], u[:-1], moves] = on[:-1]
        p[T - 1, U - 1, 0] = on[-1]                               # the final blank
        return p
    raise ValueError(name)


def lengths(N, T, U, ragged):
    """(xn, yn): full, or utterance 1 with a third of the frames and two thirds of the labels and -- in a batch of three --
    utterance 2 without labels."""
    xn = np.full((N,), T, np.int32)
    yn = np.full((N,), U - 1, np.int32)
    if ragged:
        xn[1] = max(1, T // 3)
        yn[1] = max(1, (2 * (U - 1)) // 3 - 1)
        if N > 2:
            xn[2] = T - 7
            yn[2] = 0
    return xn, yn


def batch(name, N, T, U, ragged, seed=SEED):
    """(pairs (N, T, U, 2) fp32, xn, yn): utterance n is profile(name, seed + n, Tn, Un); cells outside an utterance hold
    the profile's own values (another draw of the full size)."""
    xn, yn = lengths(N, T, U, ragged)
    pairs = np.empty((N, T, U, 2), np.float32)
    for n in range(N):
        Tn, Un = int(xn[n]), int(yn[n]) + 1
        if (Tn, Un) != (T, U):
            pairs[n] = profile(name, seed + 1000 + n, T, U)
        pairs[n, :Tn, :Un] = profile(name, seed + n, Tn, Un)
    return pairs, xn, yn


def ties_alpha(T, U):
    """The closed form of alpha on the ties profile (exact pairs -ln 2 in fp32, not ln 2 itself): log C(t+u, u) +
    (t+u) fp32(-ln 2), fp64."""
    t, u = np.meshgrid(np.arange(T), np.arange(U), indexing="ij")
    lg = np.vectorize(math.lgamma)
    return lg(t + u + 1.0) - lg(t + 1.0) - lg(u + 1.0) + (t + u) * float(NEG_LN2)


# ---- fp64 reference with the bound riding along ----
def _diagonals(T, U):
    for d in range(1, T + U - 1):
        u = np.arange(max(0, d - (T - 1)), min(U - 1, d) + 1)
        yield d - u, u


def _sweep64(sw, ew, v0, b0, constant):
    """One sweep in sweep coordinates: val[t, u] = lse(val[t-1, u] + sw[t, u], val[t, u-1] + ew[t, u]), val[0, 0] = v0 with
    bound b0; rim cells plain sums.  Returns (val, B), fp64 (T, U)."""
    T, U = sw.shape
    val = np.empty((T, U))
    B = np.empty((T, U))
    val[0, 0], B[0, 0] = v0, b0
    with np.errstate(all="ignore"):
        for t, u in _diagonals(T, U):
            ts, us = t > 0, u > 0
            tm, um = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
            skip = np.where(ts, val[tm, u] + sw[t, u], -np.inf)
            emit = np.where(us, val[t, um] + ew[t, u], -np.inf)
            v = np.logaddexp(skip, emit)
            w_s = np.where(ts, np.exp(skip - v), 0.0)
            w_e = np.where(us, np.exp(emit - v), 0.0)
            b_s = np.where(ts, B[tm, u] + EPS * np.abs(np.where(ts, skip, 0.0)), 0.0)
            b_e = np.where(us, B[t, um] + EPS * np.abs(np.where(us, emit, 0.0)), 0.0)
            val[t, u] = v
            B[t, u] = w_s * b_s + w_e * b_e + EPS * np.abs(v) + constant * EPS
    return val, B


def _edges(pairs, beta):
    """(sw, ew) of _sweep64 / emulate: the log-prob on the edge INTO sweep cell (t, u) from (t-1, u) and from (t, u-1)."""
    lpB, lpL = pairs[..., 0], pairs[..., 1]
    if beta:                                                       # mirrored: sweep cell (t', u') = (Tn-1-t, Un-1-u)
        return lpB[::-1, ::-1], lpL[::-1, ::-1]
    sw, ew = np.zeros_like(lpB), np.zeros_like(lpL)
    sw[1:] = lpB[:-1]
    ew[:, 1:] = lpL[:, :-1]
    return sw, ew


def reference(pairs, Tn, Un, lam=LAMBDA, constant=None):
    """fp64 reference and bounds of ONE utterance: ``pairs`` (T, U, 2) fp32 (its [:Tn, :Un] window is used).  A dict of
    alphas, betas, B_alpha, B_beta, grads, grad_tol (all (Tn, Un) or (Tn, Un, 2)), cost, cost_tol, ll_a, ll_tol."""
    constant = LSE_CONSTANT if constant is None else constant
    p = np.asarray(pairs[:Tn, :Un], np.float64)
    lpB, lpL = p[..., 0], p[..., 1]
    al, Ba = _sweep64(*_edges(p, False), 0.0, 0.0, constant)
    last = lpB[Tn - 1, Un - 1]
    be, Bb = _sweep64(*_edges(p, True), last, EPS * abs(last), constant)
    be, Bb = be[::-1, ::-1], Bb[::-1, ::-1]
    b00 = be[0, 0]
    ll_a = al[Tn - 1, Un - 1] + last
    # beta and its bound on the next diagonal, per channel (0 where the formula has none)
    nxt = np.zeros((Tn, Un, 2))
    Bn = np.zeros((Tn, Un, 2))
    nxt[:-1, :, 0], Bn[:-1, :, 0] = be[1:], Bb[1:]
    nxt[:, :-1, 1], Bn[:, :-1, 1] = be[:, 1:], Bb[:, 1:]
    has = np.zeros((Tn, Un, 2), bool)                              # the slots that carry a gradient
    has[:-1, :, 0] = True
    has[Tn - 1, Un - 1, 0] = True
    has[:, :-1, 1] = True
    s = al[..., None] + nxt
    x = s + p - b00
    scale = np.array([1.0, 1.0 + float(np.float32(lam))])
    with np.errstate(all="ignore"):
        g = np.where(has, -scale * np.exp(x), 0.0)
        E = Ba[..., None] + Bn + Bb[0, 0] + 4 * EPS * (np.abs(s) + abs(b00) + np.abs(x))
        tol = np.where(has, np.abs(g) * np.expm1(E) + 4 * EPS * np.abs(g), 0.0) + TINY
    return dict(alphas=al, betas=be, B_alpha=Ba, B_beta=Bb, grads=g, grad_tol=tol, cost=-b00,
                cost_tol=Bb[0, 0] + EPS * abs(b00), ll_a=ll_a, ll_tol=Ba[Tn - 1, Un - 1] + EPS * abs(ll_a))


# ---- ratios ----
def _ratios(got, ref, bound, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: a live value is not finite"
    err = np.abs(got - ref)
    pos = bound > 0
    assert (err[~pos] == 0).all(), f"{what}: a cell with bound 0 is not exact"
    q = err[pos] / bound[pos]
    if q.size == 0:
        return 0.0, 0.0
    return float(q.max()), float(np.sqrt(np.mean(q * q)))


def lattice_ratios(got, ref, bound, what="lattice"):
    """(worst, rms) of |got - ref| / bound over the live cells: ``got`` the (Tn, Un) window of a lattice."""
    return _ratios(got, ref, bound, what)


def scalar_ratio(got, ref, tol, what="cost"):
    return _ratios(np.asarray([got]), np.asarray([ref]), np.asarray([tol]), what)[0]


def gradient_ratios(got, r, what="gradients"):
    """(worst, rms) of the gradient pairs ``got`` (T, U, 2) of one utterance against ``r`` = reference(...): dead cells
    exactly 0."""
    Tn, Un = r["alphas"].shape
    got = np.asarray(got)
    dead = np.ones(got.shape[:2], bool)
    dead[:Tn, :Un] = False
    assert (got[dead] == 0).all(), f"{what}: a dead cell is not exactly 0"
    return _ratios(got[:Tn, :Un], r["grads"], r["grad_tol"], what)


def unskew(planes, T, U):
    """(N, T, U) row-major lattices from the kernels' diagonal-major planes: cell (t, u) sits in row (t + u) mod T."""
    planes = np.asarray(planes).reshape(-1, T, U)
    t, u = np.meshgrid(np.arange(T), np.arange(U), indexing="ij")
    return planes[:, (t + u) % T, u]


def batch_ratios(refs, xn, yn, alphas=None, betas=None, costs=None, ll_a=None, grads=None, what=""):
    """Ratios of a batch against its per-utterance references ``refs``: a dict of (worst, rms) per quantity given (costs
    and ll_a: worst only, as (worst, None)) -- worst the maximum over the utterances, rms over all their cells."""
    out = {}

    def fold(key, pairs_of):
        worst, ss, cnt = 0.0, 0.0, 0
        for n, r in enumerate(refs):
            Tn, Un = int(xn[n]), int(yn[n]) + 1
            w, rms, size = pairs_of(n, r, Tn, Un)
            worst = max(worst, w)
            ss += rms * rms * size
            cnt += size
        out[key] = (worst, math.sqrt(ss / max(cnt, 1)))

    if alphas is not None:
        fold("alphas", lambda n, r, Tn, Un: lattice_ratios(alphas[n][:Tn, :Un], r["alphas"], r["B_alpha"],
                                                          f"{what} alphas[{n}]") + (int((r["B_alpha"] > 0).sum()),))
    if betas is not None:
        fold("betas", lambda n, r, Tn, Un: lattice_ratios(betas[n][:Tn, :Un], r["betas"], r["B_beta"],
                                                         f"{what} betas[{n}]") + (int((r["B_beta"] > 0).sum()),))
    if grads is not None:
        fold("grads", lambda n, r, Tn, Un: gradient_ratios(grads[n], r, f"{what} grads[{n}]") + (r["grad_tol"].size,))
    if costs is not None:
        out["costs"] = (max(scalar_ratio(costs[n], r["cost"], r["cost_tol"], f"{what} costs[{n}]")
                            for n, r in enumerate(refs)), None)
    if ll_a is not None:
        out["ll_a"] = (max(scalar_ratio(ll_a[n], r["ll_a"], r["ll_tol"], f"{what} ll_a[{n}]")
                           for n, r in enumerate(refs)), None)
    return out


def dense_from_pairs(pairs, fill=-1e30):
    """(dense (N, T, U, V) fp32, labels (N, U-1) int32): the pairs scattered into dense log-probs -- column 0 the blank,
    column labels[u] = 1 + u mod (V - 1) the label, ``fill`` everywhere else."""
    N, T, U, _ = pairs.shape
    lab = (1 + np.arange(max(U - 1, 0)) % (V - 1)).astype(np.int32)
    dense = np.full((N, T, U, V), fill, np.float32)
    dense[..., 0] = pairs[..., 0]
    dense[:, :, np.arange(U - 1), lab] = pairs[:, :, :U - 1, 1]
    return dense, np.tile(lab, (N, 1))


# ---- one case = (profile, shape, ragged): inputs, references and the C oracle's result, computed once and left alone ----
@functools.lru_cache(maxsize=None)
def case(name, shape, ragged):
    """dict(pairs, xn, yn, refs (one reference per utterance), oracle (oracle.rnnt_loss_f32's dict on the pairs,
    blank=-1, FastEmit LAMBDA), oracle_ratios (batch_ratios of it))."""
    import oracle
    N, T, U = shape
    pairs, xn, yn = batch(name, N, T, U, ragged)
    refs = [reference(pairs[n], int(xn[n]), int(yn[n]) + 1) for n in range(N)]
    o = oracle.rnnt_loss_f32(pairs, None, xn, yn, blank=-1, fastemit_lambda=LAMBDA)
    ll = [o["alphas"][n, xn[n] - 1, yn[n]] + pairs[n, xn[n] - 1, yn[n], 0] for n in range(N)]       # (fp32 add)
    ratios = batch_ratios(refs, xn, yn, o["alphas"], o["betas"], o["costs"], ll, o["grads"], what=f"oracle {name} {shape}")
    for a in (pairs, xn, yn):
        a.setflags(write=False)
    return dict(pairs=pairs, xn=xn, yn=yn, refs=refs, oracle=o, oracle_ratios=ratios)


# ---- the sweeps' arithmetic in numpy ----
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def lse_kernel(skip, emit):
    """The step of lattice_step.h / lattice_single.h on fp32 arrays: max + fma(log2(u), ln2, e - (u - 1)), e =
    exp2(-|skip - emit| * log2e), u = fl(1 + e); exp2 and log2 exact and rounded once."""
    t = skip - emit
    m = -np.abs(t) * LOG2E
    e = _f32(np.exp2(m.astype(np.float64)))
    u = np.float32(1.0) + e
    l2 = _f32(np.log2(u.astype(np.float64)))
    c = e - (u - np.float32(1.0))
    l = _f32(l2.astype(np.float64) * np.float64(LN2) + c.astype(np.float64))       # (the product is exact in fp64)
    return np.maximum(skip, emit) + l


def lse_log1p_2m12(skip, emit):
    """Wrong variant (a): log(1 + e) with a relative error of 2^-12 -- a fast approximation slipped in."""
    mx = np.maximum(skip, emit)
    l = lse_kernel(skip, emit) - mx
    return mx + _f32(l.astype(np.float64) * (1.0 + 2.0 ** -12))


def lse_cut10(skip, emit):
    """Wrong variant (b): l dropped when |skip - emit| > 10."""
    mx = np.maximum(skip, emit)
    return np.where(np.abs(skip - emit) > 10, mx, lse_kernel(skip, emit)).astype(np.float32)


def lse_max(skip, emit):
    """Wrong variant (c): max instead of log-sum-exp."""
    return np.maximum(skip, emit)


def _sweep32(sw, ew, v0, lse):
    T, U = sw.shape
    val = np.empty((T, U), np.float32)
    val[0, 0] = v0
    with np.errstate(all="ignore"):
        for t, u in _diagonals(T, U):
            ts, us = t > 0, u > 0
            tm, um = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
            skip = val[tm, u] + sw[t, u]                           # (fp32 + fp32: rounded once)
            emit = val[t, um] + ew[t, u]
            v = lse(skip, emit)
            val[t, u] = np.where(ts & us, v, np.where(ts, skip, emit))      # the rim: plain sums
    return val


def emulate_sweeps(pairs, Tn, Un, lse=lse_kernel):
    """(alphas, betas) fp32 (Tn, Un) of one utterance as the kernels compute them, with ``lse`` as the step."""
    p = np.ascontiguousarray(pairs[:Tn, :Un], np.float32)
    al = _sweep32(*_edges(p, False), np.float32(0.0), lse)
    be = _sweep32(*_edges(p, True), p[Tn - 1, Un - 1, 0], lse)
    return al, be[::-1, ::-1]
