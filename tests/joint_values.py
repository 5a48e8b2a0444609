"""The fused joint kernels (csrc/joint.hip) across the logit VALUE range: input profiles whose logits are exact in fp32, the
check that they are, the bounds, and a numpy model of the kernels' per-cell arithmetic.  A helper module (like
lsm_values.py and joint_reference.py), shared by test_host_joint_values.py, test_gpu_joint_values.py and
tools/joint_value_range.py.

Exact logits.  The joint's inputs are f, g, W and b, not logits: z = W relu(f + g) + b is formed inside the kernels.  A
bound that does not grow with |b| must not charge a kernel for rounding z to fp32 at magnitude 60000, which any fp32 joint
pays.  So the base is made of small dyadic numbers: f, g integers in [-8, 8] over 4, W integers in [-8, 8] over 16, b
integers in [-16, 16] over 8 plus the profile's constant, activation relu.  Every operand fits bf16 and fp16; f + g, relu
and the cast to E are exact; every product is a multiple of 1/64 and, for H <= 128, sum |terms| + |b| < 65536: every
partial sum of z, in any order, is an integer multiple of 1/64 below 2^16, i.e. a 22-bit integer -- exact in fp32.
(assert_exact checks exactly this.)  What is left between a kernel and fp64 is its max / sum / log / exp arithmetic, and
the fp64 reference does not move under the shift.

Profiles, functions of the seeded base:

    plain                               the base
    shift+100, shift-1000, shift+60000  bias + c
    ties                                W = 0, bias = 60000 everywhere: every log-prob is -ln V
    masked                              bias = -inf on MASKED[V] (the usual way to mask a vocabulary entry)
    spread                              W * 8 (still exact): peaked rows, costs of 1e2 to 8e2
    natural-tanh, natural-relu          random non-dyadic data, W ~ 64 / sqrt(H) * randn: |z| reaches a few hundred, h stays
                                        far below 65504

MASKED[V] holds the first entry of every lane group of k_joint_fwd (v = 0, 4, 8, 12: a group's online update starts
there), an entry inside a group (6; at V >= 33 also one alone in its group, 21), a whole 16-row V block where the
vocabulary has one to spare (V = 33: block 0, so that every group meets four -inf before its first finite logit; V = 50:
block 2; V = 17 has a single full block, which must keep the blank and the labels), and the last entry of the partial
block (V - 1).  Never the blank, never a label: labels are drawn from the rest.  The blank is inside the first V block at
V = 17 (5) and beyond it at V = 33 (18) and V = 50 (17).

Out of scope, untested and not promised: cells without a finite logit, +inf, NaN, -inf on the blank or on a label an
utterance uses.

Bounds.  (a) the project's own, unchanged and not growing with |bias|: costs 1e-5 |ref| + 1e-6, gradients 1e-4 normwise and
1e-3 elementwise beyond the output dtype's rounding (test_gpu_joint_edges.py).  (b) for one log-softmax row, lsm_values.py's:
tol_j = 4 eps (|z_j - mx| + |lp_j|) + 2e-6 max(1, ln V) on a log-prob and p_j tol_j + 4 eps on a probability.

Model.  model_rows is k_joint_fwd's per-cell arithmetic in numpy -- four lane groups, each with its online max / sum over
v = 16 k + 4 q + i, their merge, log of the sum -- and the log-probs and probabilities drawn from it in two forms:
``corrected=False``  lse = mall + log(sc) in ONE fp32, lp = z - lse, p = exp(z - lse), and an online update that computes
exp(-inf - (-inf)) for a -inf entry ahead of a group's first finite one (the kernels before this module existed);
``corrected=True``   lp = (z - mall) - log(sc), p = exp of that, and a -inf entry contributes nothing."""
import numpy as np
import torch

import lsm_values as lv
from joint_reference import joint_reference
from oracle.transduce_np import transduce_batch

SHAPES = ((17, 32), (33, 64), (50, 128))                 # (V, H)
BLANK = {17: 5, 33: 18, 50: 17}
MASKED = {17: (0, 4, 8, 12, 6, 16),
          33: tuple(range(16)) + (21, 32),
          50: (0, 4, 8, 12, 6, 21) + tuple(range(32, 48)) + (49,)}
EXACT = ("plain", "shift+100", "shift-1000", "shift+60000", "ties", "masked")
RELATIVE = ("spread", "natural-tanh", "natural-relu")     # held against the unfused chain's own error
CLAIMS_EXACT = EXACT + ("spread",)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
N, T, U = 3, 9, 6                                        # U labels: g has U + 1 rows
XN, YN = (9, 7, 4), (6, 3, 0)
LAM = 0.01
COST_RTOL, COST_ATOL, NORM_TOL, ATOL_REL = 1e-5, 1e-6, 1e-4, 1e-3   # test_gpu_joint_edges.py's
QUANTUM = {name: 1.0 / 64 for name in EXACT}
QUANTUM["spread"] = 1.0 / 8


def _ints(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)


def upstream(n):
    return torch.linspace(0.25, 2.0, n) if n > 1 else torch.ones(1)


def case(name, V, H, dtype=torch.float32, n=N, t=T, u=U, xn=XN, yn=YN, seed=0):
    """Profile ``name`` at (V, H): dict of f (n,t,H), g (n,u+1,H) in ``dtype``, fp32 w (V,H) and b (V,), labels (n,u)
    int32 drawn from the entries that are neither masked nor the blank, xn, yn, act, blank, lam, up (upstream weights);
    f32 / g32 are f and g before the cast."""
    gen = torch.Generator().manual_seed(1000 * V + H + seed)
    blank = BLANK[V]
    allowed = torch.tensor([v for v in range(V) if v != blank and v not in MASKED[V]])
    labels = allowed[torch.randint(0, len(allowed), (n, u), generator=gen)].to(torch.int32)
    act = "tanh" if name == "natural-tanh" else "relu"
    if name.startswith("natural"):
        f = torch.randn(n, t, H, generator=gen)
        g = torch.randn(n, u + 1, H, generator=gen)
        w = torch.randn(V, H, generator=gen) * (64.0 / H ** 0.5)
        b = torch.randn(V, generator=gen)
    else:
        f = _ints(gen, -8, 8, (n, t, H)) / 4
        g = _ints(gen, -8, 8, (n, u + 1, H)) / 4
        w = _ints(gen, -8, 8, (V, H)) / 16
        b = _ints(gen, -16, 16, (V,)) / 8
        if name.startswith("shift"):
            b = b + float(name[5:])
        elif name == "ties":
            w = torch.zeros_like(w)
            b = torch.full_like(b, 60000.0)
        elif name == "masked":
            b[list(MASKED[V])] = float("-inf")
        elif name == "spread":
            w = w * 8
        elif name != "plain":
            raise ValueError(name)
    return dict(name=name, f=f.to(dtype), g=g.to(dtype), f32=f, g32=g, w=w, b=b, labels=labels,
                xn=torch.tensor(xn, dtype=torch.int32), yn=torch.tensor(yn, dtype=torch.int32), act=act, blank=blank,
                lam=LAM, up=upstream(n))


def cells(name, V, H, dtype=torch.float32, n=16, seed=1):
    """``n`` single-cell utterances (T = 1, no labels): the cost of each is -lp[blank] of ONE log-softmax row."""
    c = case(name, V, H, dtype, n=n, t=1, u=0, xn=(1,) * n, yn=(0,) * n, seed=seed)
    c["lam"] = 0.0
    c["up"] = torch.ones(n)
    return c


def one_cell(c, i):
    """Utterance i of ``cells(...)`` as a batch of one."""
    out = dict(c)
    for k in ("f", "g", "labels", "xn", "yn"):
        out[k] = c[k][i:i + 1].contiguous()
    out["up"] = torch.ones(1)
    return out


def args(c):
    """The positional arguments test_gpu_joint_edges.fused / reference share."""
    return c["f"], c["g"], c["w"], c["b"], c["labels"], c["xn"], c["yn"]


def logits64(c):
    """(n, t, u+1, V) fp64 logits of the case, from the values the kernels are handed (W in the activations' dtype)."""
    act = torch.tanh if c["act"] == "tanh" else torch.relu
    E = c["f"].dtype
    h = act(c["f"].float()[:, :, None] + c["g"].float()[:, None]).to(E).double()
    return h @ c["w"].to(E).double().T + c["b"].double()


def assert_exact(c):
    """The exactness the module claims of a dyadic profile: the operands are what they were before the cast to the
    activations' dtype; f + g, relu and every product are multiples of the quantum; sum |terms| + |bias| stays below 2^16,
    so every partial sum in any order is an integer multiple of the quantum of fewer than 24 bits; z rounds to itself."""
    q = QUANTUM[c["name"]]
    E = c["f"].dtype
    assert torch.equal(c["f"].float(), c["f32"]) and torch.equal(c["g"].float(), c["g32"]), "f / g change under the cast"
    assert torch.equal(c["w"].to(E).float(), c["w"]), "W changes under the cast"
    h = torch.relu(c["f"].double()[:, :, None] + c["g"].double()[:, None])
    assert torch.equal(h.to(E).double(), h), "relu(f + g) is not exact in the activations' dtype"
    w, b = c["w"].double(), c["b"].double()
    fin = torch.isfinite(b)
    for x, unit in ((h, 0.25), (w, q / 0.25), (b[fin], 0.125)):
        assert torch.equal((x / unit).round() * unit, x), "operand off its grid"
    bound = h.abs() @ w.abs().T + torch.where(fin, b.abs(), torch.zeros_like(b))
    assert float(bound.max()) < 65536.0 and 65536.0 / q <= 2 ** 24
    z = logits64(c)[..., fin]
    assert torch.equal(z.float().double(), z), "a logit is not exact in fp32"
    assert torch.equal((z / q).round() * q, z)


def reference(c, model_dz_rounding=False):
    """joint_reference on the case: costs, df, dg, dW, db in fp64 (CPU)."""
    return joint_reference(*args(c), c["act"], c["blank"], c["lam"], c["up"], model_dz_rounding=model_dz_rounding)


def torch_chain32(c):
    """torch's own fp32 chain on the CPU -- act, linear, log_softmax and their autograd in fp32 -- around the fp64
    lattice (oracle.transduce_np): costs (fp64), df, dg, dW, db (fp32)."""
    act = torch.tanh if c["act"] == "tanh" else torch.relu
    f, g, w, b = (x.detach().float().requires_grad_(True) for x in (c["f"], c["g"], c["w"], c["b"]))
    lp = torch.log_softmax(torch.nn.functional.linear(act(f[:, :, None] + g[:, None]), w, b), -1)
    costs, dlp = transduce_batch(lp.detach().double().numpy(), c["labels"].numpy(), c["xn"].numpy(), c["yn"].numpy(),
                                 c["blank"], c["lam"])
    lp.backward((torch.from_numpy(dlp) * c["up"].double()[:, None, None, None]).float())
    return torch.from_numpy(costs), f.grad, g.grad, w.grad, b.grad


# ---- one log-softmax row: lsm_values.py's bounds ----
def row_bounds(z64):
    """x64, lp64, tol of lsm_values for rows (R, V) of fp64 logits (tensor or array)."""
    x64, lp64 = lv.reference(z64)
    minf = np.isneginf(lp64)
    with np.errstate(invalid="ignore"):
        tol = lv.tolerance(x64, np.where(minf, 0.0, lp64))
    return x64, lp64, np.where(minf, 0.0, tol)              # (a masked entry is exactly -inf / 0: no tolerance)


def probability_ratio(p, lp64, tol):
    """Worst error / bound of probabilities ``p`` of rows: bound p_j tol_j + 4 eps; exactly 0 where the reference is."""
    p = np.asarray(p, np.float64).reshape(lp64.shape)
    ref = np.exp(lp64)
    assert (p[ref == 0] == 0).all(), "non-zero probability at a masked entry"
    return float(np.nan_to_num(np.abs(p - ref) / (ref * tol + 4 * lv.EPS), nan=np.inf).max())


def cost_ratio(got, ref):
    """Worst |got - ref| / (1e-5 |ref| + 1e-6) over the utterances; inf for anything not finite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.nan_to_num(np.abs(got - ref) / (COST_RTOL * np.abs(ref) + COST_ATOL), nan=np.inf).max())


# ---- k_joint_fwd's per-cell arithmetic in numpy ----
def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _exp32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return _f32(np.exp(np.asarray(a, np.float64)))


def model_rows(z, corrected):
    """(lp, p) in fp32 of rows z (R, V) -- fp32 logits -- as the kernels form them; see the module docstring."""
    z = np.asarray(z, np.float32)
    R, V = z.shape
    m = np.full((4, R), -np.inf, np.float32)
    s = np.zeros((4, R), np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for v in range(V):
            q, x = (v & 15) >> 2, z[:, v]
            gt = x > m[q]
            s_gt = _f32(s[q] * _exp32(m[q] - x)) + np.float32(1.0)
            s_le = s[q] + _exp32(x - m[q])                     # exp(-inf - (-inf)) = NaN
            if corrected:
                s_le = np.where(x > -np.inf, s_le, s[q])
            s[q] = np.where(gt, s_gt, s_le)
            m[q] = np.where(gt, x, m[q])
        mall = m.max(0)
        part = np.where(np.isneginf(m), np.float32(0.0), _f32(s * _exp32(m - mall)))
        sc = (part[0] + part[1]) + (part[2] + part[3])
        logsc = _f32(np.log(sc.astype(np.float64)))
        if corrected:
            lp = (z - mall[:, None]) - logsc[:, None]
        else:
            lp = z - (mall + logsc)[:, None]
        return lp.astype(np.float32), _exp32(lp)


def model_costs(c, corrected):
    """(costs, lp, p): the costs the fp64 lattice gives on the model's log-probs, and those log-probs / probabilities
    (n, t, u+1, V)."""
    z = logits64(c)
    lp, p = model_rows(z.reshape(-1, z.shape[-1]).numpy(), corrected)
    lp, p = lp.reshape(z.shape), p.reshape(z.shape)
    with np.errstate(invalid="ignore"):
        costs, _ = transduce_batch(lp.astype(np.float64), c["labels"].numpy(), c["xn"].numpy(), c["yn"].numpy(),
                                   c["blank"], c["lam"])
    return costs, lp, p
