"""The packed (compact=True) layout stated plainly in NumPy: what the gather and scatter kernels of csrc/compact.hip and
csrc/expand.hip must deliver, the batches that put a seam between utterances where those kernels change path, and the
comparison functions the GPU tests use (here, so that tests/test_host_compact_reference.py can show on the CPU that each of
them fails when it should).

The layout: log-probs are (STU, V) rows, utterance n owning rows [offs[n], offs[n+1]) as its own (xn[n], yn[n]+1)
row-major block; labels are packed (sum yn,).  None of the three operations does arithmetic beyond one fp32 multiply, so
every comparison against this file is bit for bit.

    pack_reference     (STU,V) log-probs -> row-major (blank, label) pairs (STU,2) and loc (STU,)
    scatter_reference  pairs of gradients, loc, per-utterance scales -> dense (STU,V) gradient rows
"""
import functools

import numpy as np

CHUNK = 1024          # cells per workgroup of k_gather_compact_linear
TILE = 32             # tile edge of k_gather_compact and k_turn_compact32
LINEAR_MAX_N = 4096   # launch_gather_compact: the linear kernel up to this many utterances, the tiled one beyond


# ---------------------------------------------------------------------------------------------------------------------
# The operations
# ---------------------------------------------------------------------------------------------------------------------
def safe_label(lab, V, blank):
    """A label outside [0, V) stands for blank (common.h)."""
    lab = int(lab)
    return lab if 0 <= lab < V else int(blank)


def pack_reference(xs, ys, xn, yn, blank):
    """Row-major pairs (STU,2) fp32 and loc (STU,) int64 of a packed batch.  Row c of utterance n is cell (t, u) of that
    utterance's (xn[n], yn[n]+1) row-major block; channel 0 is the row's blank log-prob, channel 1 the one at loc, and loc
    is `blank` on the last column, safe_label(label u of the utterance) otherwise.  Utterances with xn < 1 own no rows (their
    labels stay in ys)."""
    xs = np.asarray(xs, dtype=np.float32)
    V = xs.shape[1]
    pairs = np.zeros((xs.shape[0], 2), dtype=np.float32)
    loc = np.zeros((xs.shape[0],), dtype=np.int64)
    row = 0
    label0 = 0
    for n in range(len(xn)):
        T, U = int(xn[n]), int(yn[n]) + 1
        if T >= 1:
            for t in range(T):
                for u in range(U):
                    l = blank if u == U - 1 else safe_label(ys[label0 + u], V, blank)
                    pairs[row, 0] = xs[row, blank]
                    pairs[row, 1] = xs[row, l]
                    loc[row] = l
                    row += 1
        label0 += int(yn[n])
    assert row == xs.shape[0], "xs does not hold sum(xn * (yn + 1)) rows"
    return pairs, loc


def scatter_reference(grad_costs, grads2, loc, cum_lens, V, blank):
    """Dense (STU,V) fp32 gradient rows.  The owner of a row is the first n with cum_lens[n] > row (inclusive prefix sums
    of the cells); out[row, blank] = fl32(g.x * s_n); out[row, loc] = fl32(g.y * s_n) only when loc != blank and
    0 <= loc < V; everything else +0.0."""
    grad_costs = np.asarray(grad_costs, dtype=np.float32)
    grads2 = np.asarray(grads2, dtype=np.float32)
    STU = grads2.shape[0]
    out = np.zeros((STU, V), dtype=np.float32)
    N = len(cum_lens)
    for row in range(STU):
        n = 0
        while n < N - 1 and not int(cum_lens[n]) > row:
            n += 1
        s = grad_costs[n]
        out[row, blank] = np.float32(grads2[row, 0] * s)
        l = int(loc[row])
        if l != blank and 0 <= l < V:
            out[row, l] = np.float32(grads2[row, 1] * s)
    return out


def np_log_softmax32(x):
    x = np.asarray(x, dtype=np.float32)
    m = x.max(axis=-1, keepdims=True)
    s = np.exp(x - m, dtype=np.float32).sum(axis=-1, keepdims=True, dtype=np.float32)
    return ((x - m) - np.log(s, dtype=np.float32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# Batches
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One packed batch: xs (STU,V) fp32 log-probs, ys (sum yn,) int32, xn / yn (N,) int32, blank, FastEmit lambda."""

    def __init__(self, name, xs, ys, xn, yn, blank, lam):
        self.name, self.blank, self.lam = name, int(blank), float(lam)
        self.xs = np.ascontiguousarray(xs, dtype=np.float32)
        self.ys = np.ascontiguousarray(ys, dtype=np.int32)
        self.xn = np.ascontiguousarray(xn, dtype=np.int32)
        self.yn = np.ascontiguousarray(yn, dtype=np.int32)
        self.N, self.V = len(self.xn), self.xs.shape[1]
        self.cells = np.where(self.xn >= 1, self.xn.astype(np.int64) * (self.yn.astype(np.int64) + 1), 0)
        self.offs = np.concatenate([[0], np.cumsum(self.cells)]).astype(np.int64)
        self.label_offs = np.concatenate([[0], np.cumsum(self.yn)]).astype(np.int64)
        self.STU = int(self.offs[-1])
        self._packed = None
        assert self.xs.shape[0] == self.STU and self.ys.shape[0] == int(self.label_offs[-1])

    def subset(self, lo, hi):
        """Utterances [lo, hi) as a batch of their own."""
        return Case(f"{self.name}[{lo}:{hi}]", self.xs[self.offs[lo]:self.offs[hi]],
                    self.ys[self.label_offs[lo]:self.label_offs[hi]], self.xn[lo:hi], self.yn[lo:hi], self.blank, self.lam)

    def packed(self):
        """pack_reference of this batch (computed once)."""
        if self._packed is None:
            self._packed = pack_reference(self.xs, self.ys, self.xn, self.yn, self.blank)
        return self._packed

    def live(self):
        return self.xn >= 1

    def groups(self):
        """{(T, yn): [n, ...]} over the utterances that own rows: equal shapes go to the oracle as one unpadded batch."""
        g = {}
        for n in range(self.N):
            if self.xn[n] >= 1:
                g.setdefault((int(self.xn[n]), int(self.yn[n])), []).append(n)
        return g


def make_case(name, shapes, V=5, blank=0, lam=0.0, seed=0, bad_labels=()):
    """shapes: (xn, yn) per utterance.  Log-probs are the log-softmax of N(0,1) logits, labels are drawn from the
    vocabulary without blank; bad_labels: (utterance, u, value) entries written over them."""
    rng = np.random.RandomState(seed)
    xn = np.array([s[0] for s in shapes], dtype=np.int32)
    yn = np.array([s[1] for s in shapes], dtype=np.int32)
    assert xn.max() <= 70 and yn.max() + 1 <= 70, "lattices stay small enough that no gradient underflows"
    STU = int(sum(int(t) * (int(y) + 1) for t, y in shapes))
    xs = np_log_softmax32(rng.randn(STU, V).astype(np.float32))
    choices = np.array([v for v in range(V) if v != blank], dtype=np.int32)
    ys = choices[rng.randint(0, len(choices), size=(int(yn.sum()),))].astype(np.int32)
    label_offs = np.concatenate([[0], np.cumsum(yn)])
    for n, u, value in bad_labels:
        assert u < yn[n]
        ys[label_offs[n] + u] = value
    return Case(name, xs, ys, xn, yn, blank, lam)


def _seam_shapes(name):
    if name == "edge_exact":            # the first utterances end exactly on the first and the second chunk edge
        return [(16, 31), (8, 63), (32, 31), (5, 2), (3, 0), (7, 3)]               # 512 + 512 | 1024 | ...
    if name == "edge_off_by_one":       # ... one cell before the first edge and one cell behind it
        return [(31, 32), (1, 1), (40, 20), (3, 0), (6, 2)]                         # 1023, 1025, ...
    if name == "confetti":              # a chunk with a thousand owners, another that changes from 476 owners to one
        return [(1, 0)] * 1500 + [(40, 29)]
    if name == "empties":               # no rows at n = 0, at n = N - 1 and three times in a row -- on a chunk edge
        return [(0, 2), (30, 33), (2, 1), (0, 0), (0, 1), (0, 3), (6, 2), (5, 3), (0, 0)]   # 1020 + 4 | empties | ...
    if name == "multiple_of_chunk":     # STU = 4096: the last chunk is full
        return [(32, 31), (16, 63), (64, 31)]
    if name == "small":                 # STU = 5: one chunk, five live lanes
        return [(1, 0), (2, 1)]
    if name == "lone":                  # N = 1
        return [(37, 12)]
    if name == "no_labels":             # every utterance is one column
        return [(t, 0) for t in range(1, 51)]
    raise KeyError(name)


SEAM_CASES = ("edge_exact", "edge_off_by_one", "confetti", "empties", "multiple_of_chunk", "small", "lone", "no_labels")


@functools.lru_cache(maxsize=None)
def seam_case(name):
    """The batches that place a seam between utterances where k_gather_compact_linear's owner search changes path."""
    i = SEAM_CASES.index(name)
    case = make_case(name, _seam_shapes(name), V=5, blank=(0, 2, 4)[i % 3], lam=(0.0, 0.01)[i % 2], seed=900 + i)
    if name == "edge_exact":
        assert case.offs[2] == CHUNK and case.offs[3] == 2 * CHUNK
    if name == "edge_off_by_one":
        assert case.offs[1] == CHUNK - 1 and case.offs[2] == CHUNK + 1
    if name == "empties":
        assert case.offs[3] == CHUNK and not case.live()[[0, 3, 4, 5, case.N - 1]].any()
    if name == "multiple_of_chunk":
        assert case.STU == 4 * CHUNK
    if name == "small":
        assert case.STU == 5
    return case


# (T, U) of the utterances that straddle the 32x32 tile, and where they stand in the batch
TILE_EDGE_SHAPES = [(1, 65), (31, 33), (32, 32), (33, 32), (64, 2), (65, 1), (65, 65), (32, 33), (33, 33), (64, 32), (31, 1),
                    (1, 2)]
TILE_EDGE_N = LINEAR_MAX_N + 1
TILE_EDGE_EMPTY = (7, 3001)       # utterances without frames: one in each half of the 2048 / 2049 split


@functools.lru_cache(maxsize=None)
def tile_edge_case(blank, lam, empties=True):
    """N = 4097, one past the last batch the linear gather takes: utterances of T in 1..6, U in 1..4, a dozen whose (T, U)
    straddle the tile size first, last and mid-batch, several without labels, two without frames, one label past the
    vocabulary and one negative.  empties=False: the same batch with one frame in place of none (the bounded entry refuses a
    batch that holds an utterance without frames, so it is compared on this one)."""
    V, N = 5, TILE_EDGE_N
    rng = np.random.RandomState(4097)
    shapes = [(int(rng.randint(1, 7)), int(rng.randint(0, 4))) for _ in range(N)]
    at = [0, 1, 2, 1000, 2047, 2048, 2049, 3000, 3500, N - 3, N - 2, N - 1]
    for n, (T, U) in zip(at, TILE_EDGE_SHAPES):
        shapes[n] = (T, U - 1)
    for n in (5, 6, 1500, 2500, 4000):
        shapes[n] = (shapes[n][0], 0)
    for n in TILE_EDGE_EMPTY:
        shapes[n] = (0 if empties else 1, shapes[n][1])
    bad = [(2049, 7, V + 2), (1, 30, -3)]
    return make_case(f"tile_edges(blank={blank}, lam={lam})", shapes, V=V, blank=blank, lam=lam, seed=4097, bad_labels=bad)


def staged_case():
    """Launch bound N * Tmax * Umax past 2^20 with few live cells and an ODD total: one T = 420, U = 430 utterance sets the
    bound, the rest are tiny, the last owns no rows (the split of the staged turns reads xn[N-1] for its total and has a lone
    last cell).  Outside make_case: this lattice is long on purpose."""
    shapes = [(3, 2), (420, 429), (5, 0), (2, 3), (7, 1), (1, 4), (0, 2)]
    rng = np.random.RandomState(420)
    xn = np.array([s[0] for s in shapes], dtype=np.int32)
    yn = np.array([s[1] for s in shapes], dtype=np.int32)
    STU = int((xn.astype(np.int64) * (yn + 1)).sum())
    V = 4
    xs = np_log_softmax32(rng.randn(STU, V).astype(np.float32))
    ys = rng.randint(1, V, size=(int(yn.sum()),)).astype(np.int32)
    case = Case("staged_odd", xs, ys, xn, yn, 0, 0.01)
    assert case.N * int(xn.max()) * int(yn.max() + 1) >= 1 << 20 and case.STU % 2 == 1
    return case


def scatter_inputs(V, N, STU, blank):
    """Synthetic inputs of the scatter backward, none of them a forward's result: every value exactly representable, every
    scale distinct, loc through every vocabulary index and the four values that are none, utterances without rows first,
    last and in a row."""
    c = np.arange(STU, dtype=np.float32)
    grads2 = np.stack([c + 0.25, -(c + 0.5)], axis=1).astype(np.float32)
    scales = np.array([2.0, 0.5, 0.125, 4.0, 0.25, 1.1, 8.0] if N > 1 else [1.1], dtype=np.float32)   # 1.1: the multiply rounds
    assert len(scales) == N
    cycle = list(range(V)) + [blank, V, -1, (1 << 31) + 1]
    loc = np.array([cycle[(i + 3) % len(cycle)] for i in range(STU)], dtype=np.int64)
    if N == 1:
        lens = [STU]
    else:                                    # rows for n = 1, 4, 5 only
        a = STU // 3
        b = (STU - a) // 2
        lens = [0, a, 0, 0, b, STU - a - b, 0]
        assert N == 7
    cum_lens = np.cumsum(lens).astype(np.int32)
    assert cum_lens[-1] == STU
    return scales, grads2, loc, cum_lens


# ---------------------------------------------------------------------------------------------------------------------
# The fp32 oracle on a packed batch
# ---------------------------------------------------------------------------------------------------------------------
def oracle_packed(case):
    """oracle.rnnt_loss_f32 on the pairs of pack_reference, utterance shapes grouped so that nothing is padded: costs (N,)
    -- NaN for an utterance without rows -- and the gradient pairs (STU,2) in packing order (label channel 0 on last
    columns)."""
    import oracle
    pairs, _ = case.packed()
    costs = np.full((case.N,), np.nan, dtype=np.float32)
    grads2 = np.zeros((case.STU, 2), dtype=np.float32)
    for (T, Y), ns in case.groups().items():
        U = Y + 1
        lp = np.stack([pairs[case.offs[n]:case.offs[n + 1]].reshape(T, U, 2) for n in ns])
        ref = oracle.rnnt_loss_f32(lp, None, np.full(len(ns), T, np.int32), np.full(len(ns), Y, np.int32), blank=-1,
                                   fastemit_lambda=case.lam, scan_mode=1)
        for i, n in enumerate(ns):
            costs[n] = ref["costs"][i]
            grads2[case.offs[n]:case.offs[n + 1]] = ref["grads"][i].reshape(-1, 2)
    return costs, grads2


# ---------------------------------------------------------------------------------------------------------------------
# Comparisons (each raises AssertionError)
# ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    """The bit patterns of an array: -0.0 is not +0.0 and a NaN equals only the same NaN."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        first = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ in their bits, first at {first}: "
                             f"{got[first]!r} != {want[first]!r}")


def assert_loc(loc, case):
    """loc (STU,) against pack_reference, exactly."""
    _, want = case.packed()
    assert_same_bits(np.asarray(loc, dtype=np.int64), want, f"{case.name}: loc")


def assert_pairs(pairs, case):
    """Row-major pairs (STU,2) against pack_reference, bit for bit on every row, last columns included."""
    want, _ = case.packed()
    assert_same_bits(np.asarray(pairs, dtype=np.float32), want, f"{case.name}: pairs")


def assert_same_results(got, want, what):
    """(costs, grads2, loc) of two routes, bit for bit."""
    for g, w, part in zip(got, want, ("costs", "grads2", "loc")):
        assert_same_bits(g, w, f"{what}: {part}")


def assert_oracle(costs, grads2, case, ref=None):
    """Costs and gradient pairs against the fp32 oracle, at the tolerances this path has always been held to: rtol 1e-5
    on costs, atol 1e-4 on gradient pairs.  An utterance without rows has cost NaN."""
    ref_costs, ref_grads2 = ref if ref is not None else oracle_packed(case)
    costs = np.asarray(costs)
    live = case.live()
    assert np.isnan(costs[~live]).all(), f"{case.name}: an utterance without frames has a cost"
    np.testing.assert_allclose(costs[live], ref_costs[live], rtol=1e-5, err_msg=f"{case.name}: costs")
    np.testing.assert_allclose(np.asarray(grads2), ref_grads2, atol=1e-4, err_msg=f"{case.name}: grads2")


GUARD = np.float32(-12345.5)


def guarded_buffer_layout(V, STU, shift):
    """(size, start) in floats of a scatter output with a sentinel row before and behind it.  The front guard is a whole
    number of 16-byte groups of at least V floats so that start keeps the allocation's alignment; `shift` floats more move
    it off by that."""
    front = (V + 3) // 4 * 4 + shift
    return front + STU * V + V, front


def assert_scatter(buf, start, grad_costs, grads2, loc, cum_lens, V, blank, what):
    """A guarded output buffer (prefilled NaN between two sentinel rows) against scatter_reference: the written rows bit for
    bit -- an unwritten slot is a NaN, a -0.0 is not a +0.0 -- and both guards untouched."""
    buf = np.asarray(buf, dtype=np.float32)
    STU = np.asarray(grads2).shape[0]
    want = scatter_reference(grad_costs, grads2, loc, cum_lens, V, blank)
    assert_same_bits(buf[start:start + STU * V].reshape(STU, V), want, f"{what}: rows")
    assert_same_bits(buf[:start], np.full((start,), GUARD), f"{what}: guard before the rows")
    assert_same_bits(buf[start + STU * V:], np.full((len(buf) - start - STU * V,), GUARD), f"{what}: guard behind the rows")
