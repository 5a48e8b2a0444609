"""rnnt_loss_from_joint against float64 at the edges of its kernels' tiles (csrc/joint.hip).

Every output is compared elementwise with tests/joint_reference.py, which applies the kernels' operand rounding (h and W
in the activations' dtype E, and for bf16 / fp16 the rounding of dz to E before the second products), so the half paths
are held almost as tightly as fp32.  The axes: V against the 16-row V blocks and the 32-column pad of W^T, the blank in
and beyond the first block, H against the K steps, the 256-column H tiles, FG_MAXB and every waves-per-workgroup count of
each kernel, lengths against the 4x4 tiles, the weight kernel's split-K (several cell groups per split, empty trailing
splits, a group across two utterances), the call variants, and the c4 batch against fp64.

Tolerances: costs |got - ref| <= 1e-5 |ref| + 1e-6.  Per tensor, and per utterance for df / dg, the error beyond the
output's own rounding, e = max(|got - ref| - u_out |ref|, 0) with u_out the unit roundoff of the gradient's dtype (0 for
fp32, 2^-8 bf16, 2^-11 fp16: a returned bf16 / fp16 gradient cannot be closer than its rounding), must have
||e|| <= 1e-4 ||ref|| and max e <= 1e-3 max|ref|.  Measured worst over the sweep (normwise / elementwise): fp32 4.0e-5 /
5.5e-5, bf16 7.7e-5 / 1.2e-4, fp16 8.3e-5 / 2.0e-4.  The c4 test has its own, measured bounds.
"""
import pytest
import torch

from joint_reference import joint_reference, valid_length

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = (torch.bfloat16, torch.float16)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_IDS = ["fp32", "bf16", "fp16"]
UNIT_ROUNDOFF = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
COST_RTOL, COST_ATOL = 1e-5, 1e-6
NORM_TOL, ATOL_REL = 1e-4, 1e-3
MEASURED = []          # (case, tensor, dtype, normwise, elementwise) of every comparison, for the record


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' launch geometry, restated (joint.hip: waves_per_group, joint_w_splits, CG, LDS_PER_WG)
# ---------------------------------------------------------------------------------------------------------------------
def waves_per_group(rows, H, dtype):
    esz = 4 if dtype == torch.float32 else 2
    epf = 16 // esz
    return max(1, min(4, 81920 // (rows * (H + epf) * esz)))


def w_split_regime(N, T, U1, H, V, dtype):
    """(splits, groups, groups per split, splits with work, a group straddles two utterances) of k_joint_bwd_w."""
    cg = 16 if dtype == torch.float32 else 32
    cells = N * T * U1
    groups = -(-cells // cg)
    tiles = -(-V // 16) * -(-H // 256)
    splits = max(1, min(-(-1024 // tiles), 256, groups))
    per = -(-groups // splits)
    used = -(-groups // per)
    straddle = any((n * T * U1) % cg != 0 for n in range(1, N))
    return splits, groups, per, used, straddle


# ---------------------------------------------------------------------------------------------------------------------
# inputs, the fused call, the comparison
# ---------------------------------------------------------------------------------------------------------------------
def make(seed, N, T, U, V, H, dtype, blank, xn=None, yn=None):
    """f (N,T,H), g (N,U+1,H) in dtype; fp32 weight (V,H) and bias (V,); labels (N,U) that are never the blank and
    include V-1 and the blank's neighbours; lengths (full when not given)."""
    gen = torch.Generator().manual_seed(seed)
    f = (torch.randn(N, T, H, generator=gen) * 0.5).to(dtype)
    g = (torch.randn(N, U + 1, H, generator=gen) * 0.5).to(dtype)
    w = torch.randn(V, H, generator=gen) / H ** 0.5
    b = torch.randn(V, generator=gen) * 0.1
    labels = ((blank + 1 + torch.randint(0, V - 1, (N, U), generator=gen)) % V).to(torch.int32)
    special = [v for v in (V - 1, blank - 1, blank + 1) if 0 <= v < V and v != blank]
    for i, v in enumerate(special * N):
        if i < N * U:
            labels[i % N, (i // N) % U] = v
    xn = torch.tensor(xn if xn is not None else [T] * N, dtype=torch.int32)
    yn = torch.tensor(yn if yn is not None else [U] * N, dtype=torch.int32)
    return f, g, w, b, labels, xn, yn


def fused(f, g, w, b, labels, xn, yn, act="tanh", blank=0, lam=0.0, upstream=None, need="fgwb", reduction="none",
          average_frames=False):
    """costs (detached) and the gradients asked for (None for the others), upstream weights applied to the costs."""
    from warp_rnnt_amd.joint import rnnt_loss_from_joint
    ins = [x.detach().to(DEV) if x is not None else None for x in (f, g, w, b)]
    for x, k in zip(ins, "fgwb"):
        if x is not None and k in need:
            x.requires_grad_(True)
    out = rnnt_loss_from_joint(*ins, labels.to(DEV), xn.to(DEV), yn.to(DEV), activation=act, blank=blank,
                               fastemit_lambda=lam, reduction=reduction, average_frames=average_frames)
    (out * (upstream.to(DEV) if upstream is not None else 1.0)).sum().backward()
    return [out.detach()] + [x.grad if x is not None else None for x in ins]


def reference(f, g, w, b, labels, xn, yn, act, blank, lam, upstream, wdtype=None):
    """joint_reference with the kernels' rounding model (dz rounded for half activations); on the GPU for big cases."""
    cells = f.shape[0] * f.shape[1] * g.shape[1]
    dev = DEV if cells * w.shape[0] * w.shape[1] > 3e8 else "cpu"
    to = lambda x: x.to(dev) if x is not None else None   # noqa: E731
    out = joint_reference(to(f), to(g), to(w if wdtype is None else w.to(wdtype)), to(b), labels, xn, yn, act, blank,
                          lam, upstream, model_dz_rounding=f.dtype in HALF)
    return [x.cpu() for x in out]


def errors(got, ref):
    """The error of got beyond its own dtype's rounding, |got - ref| - u_out |ref| clamped at zero: (its norm against
    ||ref||, its largest entry against max|ref|)."""
    u = UNIT_ROUNDOFF[got.dtype]
    g64 = got.detach().double().cpu()
    excess = ((g64 - ref).abs() - u * ref.abs()).clamp_min(0.0)
    return float(excess.norm() / ref.norm()), float(excess.max() / ref.abs().max())


def compare(got, ref, name, where, norm_tol=NORM_TOL, atol_rel=ATOL_REL):
    if float(ref.abs().max()) == 0.0:
        assert torch.count_nonzero(got) == 0, (where, name)
        return
    nrm, el = errors(got, ref)
    MEASURED.append((where, name, str(got.dtype).replace("torch.", ""), nrm, el))
    assert nrm <= norm_tol, (where, name, "normwise", nrm)
    assert el <= atol_rel, (where, name, "elementwise", el)


def check_all(outs, refs, xn, yn, where, need="fgwb", has_bias=True, cost_rtol=COST_RTOL, **tol):
    c, df, dg, dw, db = outs
    rc, rf, rg, rw, rb = refs
    N, T = rf.shape[:2]
    U1 = rg.shape[1]
    for n in range(N):
        x, y = int(xn[n]), int(yn[n])
        if not valid_length(x, y, T, U1):
            assert torch.isnan(c[n]), (where, n)
            for d in (df, dg):
                if d is not None:
                    assert torch.count_nonzero(d[n]) == 0, (where, n)
            continue
        assert abs(float(c[n]) - float(rc[n])) <= cost_rtol * abs(float(rc[n])) + COST_ATOL, \
            (where, n, float(c[n]), float(rc[n]))
        for d, r, rows, k in ((df, rf, x, "f"), (dg, rg, y + 1, "g")):
            if k not in need:
                assert d is None
                continue
            assert torch.count_nonzero(d[n, rows:]) == 0, (where, n, k, "padding rows")
            compare(d[n, :rows], r[n, :rows], f"d{k}[{n}]", where, **tol)
    for d, r, k in ((dw, rw, "w"), (db, rb, "b")):
        if k in need and not (k == "b" and not has_bias):
            compare(d, r, "d" + k, where, **tol)
        else:
            assert d is None, (where, k)


def run_case(seed, N, T, U, V, H, dtype, blank, act="tanh", xn=None, yn=None, lam=0.01, bias=True, wdtype=None,
             need="fgwb", upstream=True, where="", **tol):
    f, g, w, b, labels, xn, yn = make(seed, N, T, U, V, H, dtype, blank, xn, yn)
    up = torch.linspace(0.25, 2.0, N) if upstream else None
    b = b if bias else None
    w_in = w if wdtype is None else w.to(wdtype)
    outs = fused(f, g, w_in, b, labels, xn, yn, act, blank, lam, up, need)
    assert outs[1] is None or outs[1].dtype == dtype
    assert outs[3] is None or outs[3].dtype == w_in.dtype
    refs = reference(f, g, w, b, labels, xn, yn, act, blank, lam, up, wdtype)
    check_all(outs, refs, xn, yn, f"{where} {str(dtype).replace('torch.', '')}", need, bias, **tol)
    return outs, (f, g, w_in, b, labels, xn, yn, up)


# ---------------------------------------------------------------------------------------------------------------------
# 1. V x blank x H x lengths, every dtype
# ---------------------------------------------------------------------------------------------------------------------
RESIDUES = dict(T=11, U=9, xn=[11, 10, 9, 8], yn=[9, 8, 7, 6])   # T_n and U_n+1 in every residue mod 4
SWEEP = [  # V, H, blank, act, N, T, U, xn, yn
    (2, 32, 1, "tanh", 2, 5, 2, [5, 3], [2, 1]),
    (15, 64, 0, "relu", 4, 11, 9, RESIDUES["xn"], RESIDUES["yn"]),
    (15, 288, 14, "tanh", 3, 7, 6, [7, 6, 5], [6, 3, 4]),
    (16, 416, 15, "tanh", 3, 9, 4, [9, 2, 7], [4, 4, 1]),
    (17, 256, 16, "relu", 4, 11, 9, RESIDUES["xn"], RESIDUES["yn"]),
    (17, 640, 0, "tanh", 3, 6, 5, [6, 5, 3], [5, 2, 0]),
    (31, 992, 16, "tanh", 2, 7, 5, [7, 4], [5, 3]),
    (32, 512, 31, "relu", 3, 9, 6, [9, 8, 5], [6, 6, 2]),
    (33, 1024, 16, "tanh", 2, 6, 6, [6, 5], [6, 4]),
    (33, 288, 32, "tanh", 4, 11, 9, RESIDUES["xn"], RESIDUES["yn"]),
    (64, 640, 16, "relu", 2, 7, 4, [7, 6], [4, 2]),
    (65, 416, 64, "tanh", 3, 5, 6, [5, 5, 2], [6, 1, 5]),
    (65, 32, 16, "tanh", 4, 11, 9, RESIDUES["xn"], RESIDUES["yn"]),
    (1037, 992, 16, "tanh", 2, 5, 3, [5, 4], [3, 2]),
    (1037, 64, 1036, "relu", 3, 6, 4, [6, 3, 5], [4, 4, 1]),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: f"V{c[0]}_H{c[1]}_b{c[2]}_{c[3]}")
def test_joint_sweep_against_fp64(case, dtype):
    V, H, blank, act, N, T, U, xn, yn = case
    run_case(100 + V + H, N, T, U, V, H, dtype, blank, act, xn, yn, lam=0.01 if V % 2 else 0.0,
             where=f"sweep V{V} H{H}")


def test_sweep_reaches_every_waves_per_group():
    """The sweep's H values give each kernel every workgroup size it can take (and the tests above hit each)."""
    hs = {c[1] for c in SWEEP}
    for dtype in DTYPES:
        cg = 16 if dtype == torch.float32 else 32
        want_fg = {waves_per_group(16, H, dtype) for H in range(32, 1025, 32)}
        want_w = {waves_per_group(cg, H, dtype) for H in range(32, 1025, 32)}
        assert {waves_per_group(16, H, dtype) for H in hs} == want_fg, dtype
        assert {waves_per_group(cg, H, dtype) for H in hs} == want_w, dtype
    assert {waves_per_group(16, H, torch.float32) for H in (288, 416, 512, 640)} == {4, 3, 2, 1}
    assert min(waves_per_group(16, H, torch.bfloat16) for H in range(32, 1025, 32)) == 2
    assert [waves_per_group(32, H, torch.bfloat16) for H in (416, 512, 640)] == [3, 2, 1]
    assert 1024 in hs and any(H % 256 for H in hs if H > 256)


# ---------------------------------------------------------------------------------------------------------------------
# 2. lengths against the 4x4 tiles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_joint_grid_of_one_frame(dtype):
    run_case(7, 3, 1, 5, 19, 64, dtype, 3, "tanh", [1, 1, 1], [5, 2, 0], where="T=1")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_joint_batch_without_labels(dtype):
    """labels (N,0), g (N,1,H): single-column lattices."""
    run_case(8, 3, 6, 0, 23, 96, dtype, 5, "relu", [6, 1, 4], [0, 0, 0], where="U=0")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_joint_one_cell_next_to_full(dtype):
    run_case(9, 3, 9, 7, 40, 128, dtype, 17, "tanh", [9, 1, 9], [7, 0, 7], where="xn=1,yn=0")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_joint_invalid_length_utterance(dtype):
    """xn > T: a NaN cost and exactly zero df / dg rows; the other utterances' outputs are those of the batch without
    it (df / dg to the bit, dW / db to fp32 summation order)."""
    N, T, U, V, H = 4, 9, 6, 37, 96
    outs, (f, g, w, b, labels, xn, yn, up) = run_case(10, N, T, U, V, H, dtype, 0, "tanh", [9, 12, 7, 5], [6, 3, 6, 2],
                                                      where="invalid")
    keep = [0, 2, 3]
    alone = fused(f[keep], g[keep], w, b, labels[keep], xn[keep], yn[keep], "tanh", 0, 0.01, up[keep])
    assert torch.equal(outs[0][keep], alone[0])
    assert torch.equal(outs[1][keep], alone[1]) and torch.equal(outs[2][keep], alone[2])
    for i in (3, 4):
        torch.testing.assert_close(outs[i], alone[i], rtol=1e-5, atol=1e-6 * float(alone[i].abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# 3. split-K of the weight kernel: several groups per split, empty trailing splits, a group across two utterances
# ---------------------------------------------------------------------------------------------------------------------
SPLITK = [  # N, T, U, V, H, blank, dtypes the shape is meant for
    (3, 40, 36, 16, 256, 0, (torch.float32,)),                    # fp32: 4440 cells > 4096
    (3, 47, 60, 15, 224, 14, (torch.float32,) + HALF),            # 8601 cells: > 8192 for the half kernel's 32-cell groups
    (2, 20, 10, 1037, 512, 16, (torch.float32,) + HALF),          # 8 splits, many groups each
]


@pytest.mark.parametrize("case,dtype", [(c, d) for c in SPLITK for d in c[6]],
                         ids=lambda x: f"N{x[0]}_T{x[1]}_U{x[2]}_V{x[3]}_H{x[4]}" if isinstance(x, tuple)
                         else DT_IDS[DTYPES.index(x)])
def test_joint_weight_split_k(case, dtype):
    N, T, U, V, H, blank, _ = case
    splits, groups, per, used, straddle = w_split_regime(N, T, U + 1, H, V, dtype)
    assert per >= 2 and used < splits and straddle, (splits, groups, per, used, straddle)
    xn = [T - 3 * i for i in range(N)]
    yn = [U - 5 * i for i in range(N)]
    run_case(200 + V, N, T, U, V, H, dtype, blank, "tanh", xn, yn, where=f"splitK V{V} H{H}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. call variants
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,same_dtype_weight", [(torch.float32, False), (torch.bfloat16, False),
                                                     (torch.bfloat16, True), (torch.float16, False),
                                                     (torch.float16, True)],
                         ids=["fp32", "bf16_w32", "bf16_wE", "fp16_w32", "fp16_wE"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_joint_bias_and_weight_dtype(dtype, same_dtype_weight, bias):
    run_case(11, 3, 7, 5, 33, 160, dtype, 16, "relu", [7, 4, 6], [5, 5, 2], bias=bias,
             wdtype=dtype if same_dtype_weight else None, where=f"bias{bias} wE{same_dtype_weight}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("need", ["f", "w", "b", "fg", "fgwb"])
def test_joint_requires_grad_subsets(dtype, need):
    run_case(12, 3, 6, 5, 21, 96, dtype, 20, "tanh", [6, 5, 3], [5, 1, 4], need=need, where=f"need {need}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_joint_mean_average_frames(dtype):
    N, T, U, V, H = 3, 8, 5, 29, 64
    f, g, w, b, labels, xn, yn = make(13, N, T, U, V, H, dtype, 2, [8, 5, 3], [5, 4, 0])
    outs = fused(f, g, w, b, labels, xn, yn, "tanh", 2, 0.02, reduction="mean", average_frames=True)
    weights = 1.0 / (N * xn.double())
    refs = reference(f, g, w, b, labels, xn, yn, "tanh", 2, 0.02, weights)
    want = float((refs[0] * weights).sum())
    assert abs(float(outs[0]) - want) <= COST_RTOL * abs(want)
    check_all([refs[0]] + outs[1:], refs, xn, yn, f"mean {str(dtype).replace('torch.', '')}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. misaligned views: a contiguous f, g or same-dtype weight at a 2-byte offset is the call on its aligned clone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", HALF, ids=["bf16", "fp16"])
def test_joint_misaligned_views_give_the_aligned_bits(dtype):
    from warp_rnnt_amd.joint import rnnt_loss_from_joint
    N, T, U, V, H = 3, 7, 4, 27, 96
    f, g, w, b, labels, xn, yn = make(14, N, T, U, V, H, dtype, 1, [7, 6, 3], [4, 2, 3])
    w = w.to(dtype)
    views = []
    for x in (f, g, w):
        buf = torch.empty(x.numel() + 1, dtype=dtype, device=DEV)
        buf[1:].copy_(x.reshape(-1))
        v = buf[1:].view(x.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 2
        views.append(v)
    lab, txn, tyn, bd = labels.to(DEV), xn.to(DEV), yn.to(DEV), b.to(DEV)

    def run(fx, gx, wx):
        leaves = [x.detach().requires_grad_(True) for x in (fx, gx, wx)]
        c = rnnt_loss_from_joint(*leaves, bd, lab, txn, tyn, blank=1, fastemit_lambda=0.01)
        c.sum().backward()
        return [c.detach()] + [x.grad for x in leaves]

    aligned = run(*(v.clone() for v in views))
    for i in range(3):                                  # one misaligned operand at a time, then all three
        args = [v.clone() for v in views]
        args[i] = views[i]
        for x, y in zip(run(*args), aligned):
            assert torch.equal(x, y), i
    for x, y in zip(run(*views), aligned):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the c4 batch against fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_joint_c4_against_fp64(dtype):
    """N=16, T=1500, 300 labels, V=50, H=512 (test_gpu_joint.py::test_joint_c4_size's batch) against the fp64 reference
    on the GPU, next to the unfused fp32 chain's own error to fp64.

    Measured (normwise / elementwise, beyond the output's rounding): fp32 df 2.45e-3 / 5.4e-3, dg 1.83e-3 / 2.4e-3,
    dW 1.63e-3 / 1.7e-3, db 3.5e-4; the fp32 chain 2.41e-3 / 5.6e-3, 1.79e-3 / 2.4e-3, 1.59e-3 / 1.7e-3, 2.9e-4; the two
    agree to 2.7e-4 on df.  So the error at this size is not the joint kernels': both paths share it (the fp32 loss
    lattice they both run over a 1799-step sweep), and the fused one may only add a little to it -- at most 25 % of the
    chain's error plus 1e-4.  bf16 against the rounding model: df 2.85e-3 / 9.3e-3, dg 1.73e-3 / 5.4e-3, dW 2.9e-3 /
    2.7e-3, db 1.4e-3; its ceilings are twice those.  Costs agree to 1.1e-6 (fp32) / 3.3e-6 (bf16) relative."""
    from test_gpu_joint import chain, make as make_c4
    N, T, U, V, H = 16, 1500, 300, 50, 512
    f, g, w, b, labels, xn, yn = make_c4(51, N, T, U, V, H, ragged=True)
    f, g = f.to(dtype), g.to(dtype)
    outs = fused(f, g, w, b, labels, xn, yn)
    refs = joint_reference(f.to(DEV), g.to(DEV), w.to(DEV), b.to(DEV), labels, xn, yn, "tanh", 0, 0.0,
                           model_dz_rounding=dtype in HALF)
    refs = [x.cpu() for x in refs]
    theirs = chain(f.float(), g.float(), w, b, labels, xn, yn) if dtype == torch.float32 else None
    tag = str(dtype).replace("torch.", "")
    cost_err = float(((outs[0].double().cpu() - refs[0]).abs() / refs[0].abs()).max())
    MEASURED.append((f"c4 {tag}", "costs", "float32", cost_err, cost_err))
    bf16_ceiling = {"df": (6e-3, 2e-2), "dg": (4e-3, 1.2e-2), "dw": (6e-3, 6e-3), "db": (3e-3, 3e-3)}
    for i, name in ((1, "df"), (2, "dg"), (3, "dw"), (4, "db")):
        ours = errors(outs[i], refs[i])
        MEASURED.append((f"c4 {tag}", name, str(outs[i].dtype).replace("torch.", ""), *ours))
        if theirs is not None:
            chain_err = errors(theirs[i], refs[i])
            MEASURED.append((f"c4 chain {tag}", name, "float32", *chain_err))
            MEASURED.append((f"c4 ours-vs-chain {tag}", name, "float32", *errors(outs[i], theirs[i].double().cpu())))
            for e, c, ceiling in zip(ours, chain_err, (5e-3, 1.2e-2)):
                assert e <= 1.25 * c + 1e-4 and e <= ceiling, (name, ours, chain_err)
        else:
            assert all(e <= c for e, c in zip(ours, bf16_ceiling[name])), (name, ours)
    for n in range(N):
        assert torch.count_nonzero(outs[1][n, int(xn[n]):]) == 0 and torch.count_nonzero(outs[2][n, int(yn[n]) + 1:]) == 0
    assert cost_err <= COST_RTOL, cost_err
