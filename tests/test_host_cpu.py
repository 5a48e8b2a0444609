"""CPU-side checks (no GPU): C-ABI library loads and exports every declared symbol, the drop-in
package validates arguments like the reference binding, fixtures are self-consistent, and the
multi-rank reduction is correct on a world_size-2 gloo group."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from helpers import GOLDEN, np_log_softmax32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_exported():
    """Every function include/warp_rnnt_amd.h declares is exported by the built library and
    bound by the ctypes loader (no compute calls: there is no GPU here)."""
    import warp_rnnt_amd
    from warp_rnnt_amd import _build, _lib
    _build.build()          # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    hdr = open(os.path.join(ROOT, "include", "warp_rnnt_amd.h")).read()
    declared = set(re.findall(r"\b(run_[a-z_]+|rnnt_amd_[a-z_]+)\s*\(", hdr))
    # the reference's whole C interface (core.h:29-60) is there under its own names
    assert {"run_warp_rnnt", "run_warp_rnnt_gather", "run_gather_for_compact", "run_warp_rnnt_compact",
            "run_scatter_grad_for_compact"} <= declared
    assert {"run_warp_rnnt", "run_warp_rnnt_gather", "rnnt_amd_loss", "rnnt_amd_expand_grads",
            "rnnt_amd_log_softmax", "rnnt_amd_gather", "rnnt_amd_workspace_size"} <= declared
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    L = warp_rnnt_amd.load()
    for name in declared:
        assert getattr(L, name) is not None
    assert L.rnnt_amd_version() >= 100
    # pure host-side entry point: sizes
    assert L.rnnt_amd_workspace_size(16, 1500, 300) >= 16 * 1500 * 300 * 16
    assert L.rnnt_amd_workspace_size(1, 0, 3) == 0          # invalid dims are rejected
    syms = subprocess.check_output(["nm", "-D", "--defined-only", warp_rnnt_amd.lib_path()]).decode()
    for name in declared:
        assert re.search(r"\bT " + name + r"\b", syms), name


def test_the_only_setting_is_a_debug_kernel_pin_and_sizes_do_not_depend_on_it():
    """Round 6: one arithmetic, no route setting (rnnt_amd_set_lattice and the per-call *_ex entries are gone).  What is
    left is rnnt_amd_debug_set_lattice_kernel / warp_rnnt_amd.debug.set_lattice_kernel: host-side state only (one atomic),
    so it is testable here.  The workspace size is a function of the shape alone."""
    import warp_rnnt_amd
    from warp_rnnt_amd import debug
    L = warp_rnnt_amd.load()
    for gone in ("rnnt_amd_set_lattice", "rnnt_amd_get_lattice", "rnnt_amd_loss_ex", "rnnt_amd_loss_compact_ex",
                 "rnnt_amd_set_logdomain_kernel"):
        assert not hasattr(L, gone), gone
    syms = subprocess.check_output(["nm", "-D", "--defined-only", warp_rnnt_amd.lib_path()]).decode()
    assert "lattice_pd" not in syms and "k_lattice_pd" not in syms          # the second arithmetic is not in the library
    # hand-over rings are reserved for every shape with more than one column block (one granule per diagonal and boundary)
    # and for no others
    cells = lambda n, t, u: n * t * u * 16
    assert L.rnnt_amd_workspace_size(16, 1500, 64) - cells(16, 1500, 64) < 1 << 16
    assert 1 << 20 < L.rnnt_amd_workspace_size(16, 1500, 300) - cells(16, 1500, 300) < 1 << 22
    wide = L.rnnt_amd_workspace_size(2, 100, 1100) - cells(2, 100, 1100)
    assert 2 * 2 * 17 * (1199 + 8) * 8 <= wide < 1 << 20
    size = L.rnnt_amd_workspace_size(16, 1500, 300)
    try:
        assert debug.set_lattice_kernel("wd") == "auto" and L.rnnt_amd_debug_get_lattice_kernel() == 2
        assert L.rnnt_amd_workspace_size(16, 1500, 300) == size
        assert debug.set_lattice_kernel("ws") == "wd"
        assert L.rnnt_amd_debug_set_lattice_kernel(9) == -1 and L.rnnt_amd_debug_get_lattice_kernel() == 1
        with debug.lattice_kernel("wl"):
            assert debug.get_lattice_kernel() == "wl" and L.rnnt_amd_workspace_size(16, 1500, 300) == size
        assert debug.get_lattice_kernel() == "ws"
        with pytest.raises(ValueError, match="unknown lattice kernel"):
            debug.set_lattice_kernel("fast")
    finally:
        debug.set_lattice_kernel("auto")
    assert L.rnnt_amd_workspace_size_compact(4, 4 * 700 * 200, 700, 200) > L.rnnt_amd_workspace_size_compact(4, 4 * 700 * 200, 700, 64)


def test_kernel_pin_initial_value_comes_from_the_environment():
    code = ("import sys; sys.path.insert(0, %r); import torch; from warp_rnnt_amd import debug; print(debug.get_lattice_kernel())" % ROOT)
    for env, want in (({}, "auto"), ({"RNNT_DEBUG_LATTICE_KERNEL": "ws"}, "ws"), ({"RNNT_DEBUG_LATTICE_KERNEL": "wl"}, "wl")):
        e = {k: v for k, v in os.environ.items() if k != "RNNT_DEBUG_LATTICE_KERNEL"}
        e.update(env)
        out = subprocess.run([sys.executable, "-c", code], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             timeout=300)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        assert out.stdout.decode().split()[-1] == want


def test_missing_library_fails_loudly(monkeypatch):
    from warp_rnnt_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_LIB_NAME", "libdoes_not_exist.so")
    with pytest.raises(RuntimeError, match="has not been built"):
        _lib.load()


def test_product_never_imports_oracle():
    """The product packages must not reference the oracle (or any CPU fallback)."""
    for pkg in ("warp_rnnt", "warp_rnnt_amd"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, pkg)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp")):
                    src = open(os.path.join(dirpath, f)).read()
                    assert not re.search(r"^\s*(import|from)\s+oracle", src, re.M), os.path.join(dirpath, f)
                    assert "librnnt_oracle" not in src


def test_argument_validation_on_cpu():
    """Order and texts of binding.cpp:32-51 that can be observed without a GPU (test.py:15-32)."""
    import warp_rnnt._C as core
    xs = torch.tensor([], dtype=torch.float32)
    e = torch.tensor([], dtype=torch.int)
    nc = torch.tensor(np.zeros((4, 3, 2, 1)), dtype=torch.float32).transpose(0, 1)
    with pytest.raises(RuntimeError, match="xs must be contiguous"):
        core.rnnt_loss(nc, e, e, e)
    with pytest.raises(RuntimeError, match="xs must be located in the CUDA"):
        core.rnnt_loss(xs, e, e, e)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        core.rnnt_loss(xs, torch.tensor([], dtype=torch.long), e, e)
    with pytest.raises(RuntimeError, match="xs must be a Float tensor"):
        core.rnnt_loss(xs.half(), e, e, e)
    with pytest.raises(RuntimeError, match="xn must be a Int tensor"):
        core.rnnt_loss(xs, e, e.long(), e)


def test_wrapper_asserts_and_reduction_errors():
    import warp_rnnt
    lp = torch.zeros((1, 2, 2, 3))
    ys = torch.zeros((1, 1), dtype=torch.int)
    n = torch.ones((1,), dtype=torch.int)
    with pytest.raises(AssertionError):
        warp_rnnt.rnnt_loss(lp, ys, n, n, reduction="avg")
    with pytest.raises(AssertionError):
        warp_rnnt.rnnt_loss(lp, ys, n, n, blank=0.0)
    with pytest.raises(AssertionError):
        warp_rnnt.rnnt_loss(lp, ys, n, n, gather=1)
    with pytest.raises(RuntimeError, match="located in the CUDA"):
        warp_rnnt.rnnt_loss(lp, ys, n, n)          # no CPU fallback


def test_wrapper_fixtures_self_consistent():
    """The fixtures generated from the reference's own wrapper: for gather=True the native op
    receives the (N,T,U,2) [blank,label] gather with blank=-1 (__init__.py:118-128)."""
    fx = np.load(os.path.join(GOLDEN, "wrapper_fixtures.npz"))
    lp = np_log_softmax32(fx["logits"])
    seen_gather = 0
    for row in fx["cases"]:
        key, blank, gather, reduction, avg, lam, native_blank = row.split(";")
        blank, gather, native_blank = int(blank), int(gather), int(native_blank)
        nin = fx[key + "_native_in"]
        if gather:
            seen_gather += 1
            assert native_blank == -1 and nin.shape[-1] == 2
            np.testing.assert_allclose(nin, oracle.gather_f32(lp, fx[key + "_labels"], blank), atol=1e-6)
        else:
            assert native_blank == blank
            np.testing.assert_allclose(nin, lp, atol=1e-6)
    assert seen_gather > 0


def test_shard_bounds():
    from warp_rnnt_amd.distributed import shard_bounds
    for n in (0, 1, 7, 16, 128):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1


WORKER = r'''
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch, torch.distributed as dist
import oracle
from helpers import make_case, np_log_softmax32
from warp_rnnt_amd.distributed import reduce_costs, shard_bounds
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank, world = dist.get_rank(), dist.get_world_size()
logits, labels, xn, yn = make_case(3, 5, 9, 4, 6, ragged=True)       # global batch of 5 on 2 ranks: 3 + 2
lp = np_log_softmax32(logits)
full = oracle.rnnt_loss_f32(lp, labels, xn, yn)
lo, hi = shard_bounds(5, rank, world)
mine = oracle.rnnt_loss_f32(lp[lo:hi], labels[lo:hi], xn[lo:hi], yn[lo:hi])
np.testing.assert_array_equal(mine["costs"], full["costs"][lo:hi])       # utterances are independent
costs = torch.tensor(mine["costs"], requires_grad=True)
for red in ("sum", "mean"):
    loss, glob = reduce_costs(costs, red)
    want = full["costs"].sum() if red == "sum" else full["costs"].mean()
    np.testing.assert_allclose(glob.item(), want, rtol=1e-6)
    g, = torch.autograd.grad(loss, costs)
    np.testing.assert_allclose(g.numpy(), np.full(hi - lo, 1.0 if red == "sum" else 1.0 / 5), rtol=1e-6)
    # sum over ranks of the local losses is the global loss
    t = loss.detach().clone(); dist.all_reduce(t)
    np.testing.assert_allclose(t.item(), want, rtol=1e-6)
_, allc = reduce_costs(costs, "none")
np.testing.assert_array_equal(allc.numpy(), full["costs"])
_, allc = reduce_costs(costs, "none", n_global=5)                       # sizes known: one all-gather, no read-back
np.testing.assert_array_equal(allc.numpy(), full["costs"])
try:
    reduce_costs(costs, "none", n_global=7); raise SystemExit("a wrong n_global must be rejected")
except ValueError:
    pass
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
'''


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_rank_reduction_gloo(tmp_path):
    """world_size 2 on CPU (gloo): sharding + the scalar exchange of the multi-GPU path."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT))
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} ok" in o


def test_bench_configs_match_baseline_json():
    """bench.py's workloads are BASELINE.json's configs[1..4] (per rank for the 8-GPU rows)."""
    import importlib.util
    import json
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cfgs = json.load(open(os.path.join(root, "BASELINE.json")))["configs"]
    for name, text in zip(("c2", "c3", "c4", "c5"), cfgs[1:5]):
        n, t, u, v = (int(re.search(rf"\b{k}=(\d+)", text).group(1)) for k in ("N", "T", "U", "V"))
        ranks = 8 if "8×MI355X" in text or "8xMI355X" in text else 1
        N, T, U, V, gather, lam, _ = bench.CONFIGS[name]
        assert (N * ranks, T, U, V) == (n, t, u, v), (name, text)
        assert gather == ("gather=True" in text or "gather path" in text), (name, text)
        if "fastemit_lambda=" in text:
            assert abs(lam - float(re.search(r"fastemit_lambda=([0-9.]+)", text).group(1))) < 1e-9
    # the default workload is the one the metric is quoted on (configs[3] per rank, README.md:51)
    assert bench.parse.__defaults__ is None and "c4" in bench.CONFIGS


def test_bench_dump_outputs_writes_a_fixed_sample_in_float(tmp_path):
    """bench.py --dump-outputs (on CPU tensors): the costs whole, the log-probs whole when small and otherwise the same
    seeded sample of flat indices every time, float32 / float64 only, within 64 MiB."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    small = {"costs": torch.arange(3, dtype=torch.float32), "log_probs": -torch.rand((3, 4, 5, 6))}
    assert bench.dump_outputs(str(tmp_path / "s"), small, 0, 1) == ["costs", "log_probs"]
    np.testing.assert_array_equal(np.load(tmp_path / "s" / "log_probs.npy"), small["log_probs"].numpy())
    big = {"costs": torch.zeros(2), "log_probs": torch.randn((2, 2 * bench.DUMP_SAMPLE))}
    for d in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / d), big, 1, 2) == ["costs_rank1", "log_probs_index_rank1",
                                                                     "log_probs_rank1"]
    files = sorted(os.listdir(tmp_path / "a"))
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(x, y)
    idx = np.load(tmp_path / "a" / "log_probs_index_rank1.npy")
    assert 0 < idx.size <= bench.DUMP_SAMPLE // 2 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "log_probs_rank1.npy"),
                                  big["log_probs"].reshape(-1)[torch.from_numpy(idx.astype(np.int64))].numpy())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20


def test_bench_self_launches_ranks_gloo_dry():
    """`python bench.py --gpus 2` with no launcher around it re-executes itself under torch.distributed.run
    (one rank per GPU, 127.0.0.1 rendezvous) -- what the driver's SCALE runs invoke.  CPU rehearsal: gloo, no
    kernels; the JSON line must come from rank 0 of a 2-rank group after a real all-reduce."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                          "--dry", "--steps", "2", "--warmup", "1"], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, text
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2 and rec["dry"] is True
    assert rec["reduced_scalar"] == 3.0            # 1 + 2: both ranks contributed
    # a world size that contradicts --gpus is refused, not silently accepted
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry"],
                         env=dict(env, WORLD_SIZE="1", RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         timeout=120)
    assert bad.returncode != 0 and b"launcher started 1 rank" in bad.stdout


def test_bench_eight_ranks_weak_and_strong_gloo_dry():
    """What the driver's SCALE run does on an 8-GPU node, rehearsed on CPU: `bench.py --gpus 8` starts eight ranks,
    every rank joins the group, the scalar reduction sees all eight, the per-rank time spread is gathered; and with
    --global-batch 128 (BASELINE.json configs[3] as a strong-scaling run) the shards add up to the global batch."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    for extra, scaling, owned in (([], "weak", 8 * 16), (["--global-batch", "128"], "strong", 128),
                                  (["--global-batch", "100"], "strong", 100)):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--backend", "gloo", "--dry",
                              "--steps", "2", "--warmup", "1"] + extra, env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, timeout=600)
        text = out.stdout.decode()
        assert out.returncode == 0, text
        lines = [ln for ln in text.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, text
        rec = json.loads(lines[0])
        assert rec["n_gpus"] == 8 and rec["rccl_ranks"] == 8 and rec["dry"] is True and rec["scaling"] == scaling
        assert rec["reduced_scalar"] == 36.0                      # 1 + ... + 8
        assert rec["utterances_owned_by_all_ranks"] == owned
        lo, hi = rec["ms_per_step_rank_min_max"]
        assert 0 < lo <= hi


def test_compiled_binding_is_built_and_checks_arguments_like_the_reference():
    """warp_rnnt._C_native (csrc/binding.cpp): the reference's check order and texts (binding.cpp:32-51, test.py:15-32)
    come from TORCH_CHECK there; whatever can be observed without a GPU is observed here."""
    import warp_rnnt._C as core
    assert core._native is not None, "warp_rnnt/_C_native.so has not been built (_build.build_binding)"
    nat = core._native
    for fn in ("rnnt_loss", "rnnt_loss_gather", "rnnt_loss_gather_backward", "log_softmax", "library_version"):
        assert hasattr(nat, fn)
    xs = torch.tensor([], dtype=torch.float32)
    e = torch.tensor([], dtype=torch.int)
    nc = torch.tensor(np.zeros((4, 3, 2, 1)), dtype=torch.float32).transpose(0, 1)
    with pytest.raises(RuntimeError, match="xs must be contiguous"):
        nat.rnnt_loss(nc, e, e, e)
    with pytest.raises(RuntimeError, match="xs must be located in the CUDA"):
        nat.rnnt_loss(xs, e, e, e)
    with pytest.raises(RuntimeError, match="ys must be a Int tensor"):
        nat.rnnt_loss(xs, torch.tensor([], dtype=torch.long), e, e)
    with pytest.raises(RuntimeError, match="xs must be a Float tensor"):
        nat.rnnt_loss(xs.half(), e, e, e)
    # keyword names of the reference's module (binding.cpp:250-254; used as kwargs at __init__.py:13-18)
    with pytest.raises(RuntimeError, match="located in the CUDA"):
        nat.rnnt_loss(xs=xs, ys=e, xn=e, yn=e, blank=0, fastemit_lambda=0.0)


def test_reference_binding_links_against_this_library():
    """INTEGRATION.md section 1 says the reference's own pytorch_binding/binding.cpp links whole against
    include/warp_rnnt_amd.h + libwarp_rnnt_amd.so (binding.cpp:85-99 run_warp_rnnt[_gather], :170,:197,:241 the
    three compact entry points).  build() compiles it, edited as that section says, with every symbol required to
    resolve (-Wl,--no-undefined), into oracle/_ref/ (oracle/ref_binding.py); here the module is imported."""
    import importlib.util
    from oracle import ref_binding
    if os.access(ref_binding.reference_binding(), os.R_OK):
        from warp_rnnt_amd import _build
        assert ref_binding.build(_build.build()) == ref_binding.MODULE
    elif not os.path.exists(ref_binding.MODULE):
        pytest.skip("oracle/_ref/_C_ref.so not built: build() found no reference checkout to build it from")
    text = open(ref_binding.SOURCE).read()
    for old, new in ref_binding.EDITS:
        assert new in text and old not in text
    for name in ref_binding.ENTRY_POINTS:
        assert name in text                      # the five core.h entry points are what it calls
    # the module imports and carries the reference's three ops; its argument checks run before any device work
    spec = importlib.util.spec_from_file_location("_C_ref", ref_binding.MODULE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for fn in ("rnnt_loss", "rnnt_loss_compact", "rnnt_loss_compact_backward"):      # binding.cpp:250-266
        assert hasattr(mod, fn), dir(mod)
    e = torch.tensor([], dtype=torch.int)
    with pytest.raises(RuntimeError, match="xs must be located in the CUDA"):
        mod.rnnt_loss(torch.tensor([], dtype=torch.float32), e, e, e, 0, 0.0)


def test_committed_traffic_file_has_what_bench_reads():
    """bench.py labels `roofline.traffic` / `roofline_gather.traffic` with the committed counter collection
    (profiles/hbm_traffic.json, written by tools/summarise_profiles.py): the entries it looks up must be there, each with
    its source, and within a factor two of the algorithmic bytes they are compared with."""
    import json
    doc = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    algorithmic = {"c4": 2.88e9, "c3": 3.84e9, "c4_gather": 1.31e9 + 0.0576e9}
    for key, alg in algorithmic.items():
        rec = doc[key]
        assert rec["source"] and rec["kernel"], key
        assert 0.9 * alg < rec["traffic_bytes"] < 2.0 * alg, (key, rec["traffic_bytes"])



def test_in_place_reloads_of_the_lattice_kernels_are_not_touched_before_their_wait():
    """tools/check_inplace_reloads.py on the ISA hipcc generates for csrc/lattice_wd.hip: between an in-place LDS reload of
    a block's pairs / seeds (inline assembly the compiler does not count) and the `s_waitcnt lgkmcnt(0)` in front of the
    block barrier, nothing -- in particular nothing the compiler added: a copy at a loop head, a temporary -- reads or
    writes the registers being refilled.  And the checker itself notices when something does."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_inplace_reloads as chk
    path = chk.compile_to_asm(os.path.join(ROOT, "warp_rnnt_amd", "csrc", "lattice_wd.hip"))
    kernels, reloads, bad = chk.check(path)
    assert kernels >= 4 and reloads >= 200, (kernels, reloads)      # (wd + wl, padded + compact; 24 per fast block at least)
    assert not bad, bad[:5]
    text = open(path).read()
    m = re.search(r"(ds_read2st64_b64 v\[(\d+):\d+\], v\d+ offset0:0 offset1:1\n\t;;#ASMEND\n)", text)
    assert m
    broken = text.replace(m.group(1), m.group(1) + "\tv_mov_b32_e32 v255, v%s\n" % m.group(2), 1)
    bpath = path + ".broken.s"
    with open(bpath, "w") as f:
        f.write(broken)
    assert len(chk.check(bpath)[2]) == 1
    # the same ISA under the wait-state walk: clean as generated; and the ONE instruction the compiler places between two
    # hand-written steps (the store of the cell's value) is what keeps the DPP read two wait states behind its operand --
    # take it out and the walk says so
    nk, ni, found = chk.check_hazards(path)
    assert nk >= 8 and ni > 50000 and not found, found[:5]
    m = re.search(r"(\t;;#ASMEND\n)\tds_write_b32 v\d+, v\d+\n(\t;;#ASMSTART\n\tv_(?:sub_f32|mov_b32)_dpp )", text)
    assert m
    with open(bpath, "w") as f:
        f.write(text.replace(m.group(0), m.group(1) + m.group(2), 1))
    found = chk.check_hazards(bpath)[2]
    assert found and all(f[4] and "DPP read" in f[3] for f in found), found[:5]


def test_the_build_refuses_a_planted_reload_violation(monkeypatch):
    """`_build.build()` checks the ISA of the object it is about to link (warp_rnnt_amd/_isa_check.py) and FAILS when an
    instruction touches a register whose in-place LDS reload may still be in flight -- the family of round 5's two silent
    wrong-answer bugs.  The `planted_violation` variant ends the hand-written blocks with `lgkmcnt(2)` instead of
    `lgkmcnt(0)` (two reloads left in flight across the barrier: exactly the first of those bugs): build() must raise,
    leave no object and no library behind, and the default build must be one that went through the same gate."""
    from warp_rnnt_amd import _build, _isa_check
    assert "lattice_wd.hip" in _build.RELOAD_CHECKED and "lattice_wd.hip" in _build.SOURCES
    monkeypatch.setattr(_build, "SOURCES", ["lattice_wd.hip"])      # (the one translation unit with such reloads)
    objdir = os.path.join(os.path.dirname(_build.LIB), "build_planted_violation")
    with pytest.raises(_isa_check.ReloadCheckError, match="reload may still be in flight"):
        _build.build(variant="planted_violation")
    assert not os.path.exists(os.path.join(objdir, "lattice_wd.o"))
    assert not os.path.exists(_build.variant_path("planted_violation"))
    # ... and the shipped library's own object carries the mark of a passed check for exactly its sources and flags
    monkeypatch.undo()
    _build.build()
    mark = os.path.join(os.path.dirname(_build.LIB), "build", "lattice_wd.o.reloads_ok")
    if os.path.exists(os.path.join(os.path.dirname(_build.LIB), "build", "lattice_wd.o")):   # (built here, not shipped prebuilt)
        with open(mark) as f, open(_build.LIB + ".fingerprint") as g:
            assert f.read() == g.read()


def test_compile_time_switches_are_the_kept_builds_only():
    """Every RNNT_* macro the native sources test in a preprocessor conditional belongs to a build that has a user: the
    four _build.VARIANTS and the diagnostics build of tools/wd_trace.py (RNNT_WD_STATS).  A new experiment switch is added
    here on purpose or goes through ab_getenv (common.h)."""
    from warp_rnnt_amd import _build
    allowed = {"RNNT_AB_KNOBS", "RNNT_WD_SPIN_LIMIT", "RNNT_LATTICE_LEGACY", "RNNT_PRECISE_LIBM",
               "RNNT_PLANT_RELOAD_VIOLATION", "RNNT_WD_STATS"}
    found = {}
    for d in (_build.CSRC, os.path.join(ROOT, "include")):
        for name in sorted(os.listdir(d)):
            if not name.endswith((".h", ".hip", ".cpp")):
                continue
            with open(os.path.join(d, name)) as f:
                text = f.read().replace("\\\n", " ")
            conds = re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", text, re.M)
            conds += re.findall(r"\bdefined\s*\(?\s*(RNNT_\w+)", text)
            for c in conds:
                for m in re.findall(r"\bRNNT_\w+", c):
                    found.setdefault(m, name)
    assert set(found) == allowed, {m: found.get(m) for m in set(found) ^ allowed}
    assert set(_build.VARIANTS) == {"precise", "short_spin", "ab", "planted_violation"}


def test_the_build_refuses_inline_assembly_stores_of_more_than_64_bits(tmp_path):
    """gfx950: a VMEM store of more than 64 bits reads its data registers up to two wait states after it issues; the compiler
    pads its own, not one inside `asm` (found by tools/ubench/lsm_store_policy.hip's bit check in round 6).  The build
    refuses such a store in the library's sources unless it carries its own `s_nop`; the shipped sources have none."""
    from warp_rnnt_amd import _build, _isa_check
    srcs = [os.path.join(_build.CSRC, x) for x in list(_build.SOURCES) + list(_build.HEADERS)]
    _isa_check.require_no_wide_asm_stores(srcs)
    bad = tmp_path / "bad.hip"
    bad.write_text('__device__ void f(float4* p, float4 v) {\n'
                   '    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");\n'
                   '    // asm volatile("global_store_dwordx4 %0, %1, off" in a comment does not count\n'
                   '    asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");\n'
                   '    asm volatile("buffer_store_dwordx3 %0, %1, %2, 0 offen"\n'
                   '                 ::"v"(v), "v"(0), "s"(0) : "memory");\n'
                   '    asm volatile("global_store_dwordx4 %0, %1, off sc1\\n\\ts_nop 1" ::"v"(p), "v"(v) : "memory");\n}\n')
    assert [ln for ln, _ in _isa_check.wide_asm_stores(str(bad))] == [2, 5]
    with pytest.raises(_isa_check.ReloadCheckError, match="more than 64 bits"):
        _isa_check.require_no_wide_asm_stores(srcs + [str(bad)])


def test_the_isa_walk_sees_the_wait_state_hazards_around_inline_assembly(tmp_path):
    """_isa_check's third rule on hand-made ISA: each hazard alone, its padded form, a hazard that only exists along a
    loop's back edge, and that compiler-only findings are reported but not fatal.  (The shipped objects pass the same
    walk inside _build.build(): HAZARD_CHECKED.)"""
    from warp_rnnt_amd import _build, _isa_check

    def isa(body):
        f = tmp_path / f"k{abs(hash(body))}.s"
        f.write_text("_Z1kv:\n" + body + "\ts_endpgm\n")
        return str(f)

    A, E = "\t;;#ASMSTART\n", "\t;;#ASMEND\n"
    dpp = "\tv_mov_b32_dpp v4, v1 wave_shr:1 row_mask:0xf bank_mask:0xf\n"
    # the compiler's instruction one slot in front of an inline DPP read of its result
    bad = isa("\tv_add_f32_e32 v1, v2, v3\n\tds_write_b32 v9, v8\n" + A + dpp + E)
    assert [f[3][:8] for f in _isa_check.check_hazards(bad)[2]] == ["DPP read"]
    with pytest.raises(_isa_check.AsmHazardError, match="DPP read of v1 1 wait"):
        _isa_check.require_no_asm_hazards(bad)
    # two slots: fine; s_nop 1 counts two; only the DPP operand (first source) matters
    for ok in ("\tv_add_f32_e32 v1, v2, v3\n\tds_write_b32 v9, v8\n\tv_add_f32_e32 v7, v2, v3\n" + A + dpp + E,
               "\tv_add_f32_e32 v1, v2, v3\n\ts_nop 1\n" + A + dpp + E,
               "\tv_add_f32_e32 v1, v2, v3\n" + A + "\tv_sub_f32_dpp v2, v50, v1 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n" + E):
        assert _isa_check.require_no_asm_hazards(isa(ok))[2] == []
    # a transcendental's result in the next slot; one instruction between is enough; trans -> trans is no hazard
    with pytest.raises(_isa_check.AsmHazardError, match="transcendental"):
        _isa_check.require_no_asm_hazards(isa(A + "\tv_exp_f32 v5, v1\n\tv_add_f32 v6, 1.0, v5\n" + E))
    _isa_check.require_no_asm_hazards(isa(A + "\tv_exp_f32 v5, v1\n\tv_max_f32 v7, v1, v2\n\tv_add_f32 v6, 1.0, v5\n" + E))
    _isa_check.require_no_asm_hazards(isa(A + "\tv_exp_f32 v5, v1\n\tv_log_f32 v6, v5\n" + E))
    # the wide store: the finding of tools/ubench/lsm_store_policy.hip
    with pytest.raises(_isa_check.AsmHazardError, match="more than 64 bits"):
        _isa_check.require_no_asm_hazards(isa(A + "\tglobal_store_dwordx4 v[12:13], v[4:7], off sc1\n" + E +
                                              "\ts_or_b64 exec, exec, s[10:11]\n\tv_max_f32_e32 v4, v19, v19\n"))
    _isa_check.require_no_asm_hazards(isa(A + "\tglobal_store_dwordx4 v[12:13], v[4:7], off sc1\n\ts_nop 1\n" + E +
                                          "\tv_max_f32_e32 v4, v19, v19\n"))
    _isa_check.require_no_asm_hazards(isa(A + "\tglobal_store_dwordx2 v[12:13], v[4:5], off sc1\n" + E + "\tv_max_f32_e32 v4, v19, v19\n"))
    # the LDS-DMA loads: descriptor / offset / LDS base out of v_readfirstlane need 5 wait states before a VMEM read; M0 needs 1
    dma = "\tbuffer_load_dwordx4 v1, s[4:7], s9 offen sc1 lds\n"
    with pytest.raises(_isa_check.AsmHazardError, match="VMEM read of s9 4 wait"):
        _isa_check.require_no_asm_hazards(isa("\tv_readfirstlane_b32 s9, v3\n\ts_nop 1\n" + A + "\ts_mov_b32 m0, s3\n\ts_nop 0\n" + dma + E))
    with pytest.raises(_isa_check.AsmHazardError, match="VMEM read of s6"):
        _isa_check.require_no_asm_hazards(isa("\tv_readfirstlane_b32 s6, v3\n" + A + "\ts_mov_b32 m0, s3\n\ts_nop 0\n" + dma + E))
    with pytest.raises(_isa_check.AsmHazardError, match="behind the write of M0"):
        _isa_check.require_no_asm_hazards(isa(A + "\ts_mov_b32 m0, s3\n" + dma + E))
    _isa_check.require_no_asm_hazards(isa("\tv_readfirstlane_b32 s9, v3\n\ts_nop 2\n" + A + "\ts_mov_b32 m0, s3\n\ts_nop 0\n" + dma + E))
    # (a scalar instruction that overwrites the SGPR in between makes the VALU write dead: a carry-out nobody reads)
    _isa_check.require_no_asm_hazards(isa("\tv_mad_u64_u32 v[22:23], s[10:11], v9, s54, v[2:3]\n\ts_mov_b32 s10, 0\n\ts_movk_i32 s11, 0x3000\n" + A +
                                          "\ts_mov_b32 m0, s11\n\ts_nop 0\n\tbuffer_load_dwordx4 v22, s[36:39], s10 offen lds\n" + E))
    # only along the back edge: the loop's last instruction writes what its first instruction reads through DPP
    loop = isa("\tv_mov_b32_e32 v1, 0\n\ts_nop 4\n.LBB0_1:\n" + A + dpp + "\tv_add_f32 v9, v4, v4\n\tv_add_f32 v1, v4, v9\n" + E +
               "\ts_cbranch_scc1 .LBB0_1\n")
    with pytest.raises(_isa_check.AsmHazardError, match="DPP read of v1 1 wait"):
        _isa_check.require_no_asm_hazards(loop)
    # between two compiler instructions: the model's problem, not the build's
    nk, ni, rest = _isa_check.require_no_asm_hazards(isa("\tv_exp_f32_e32 v5, v1\n\tv_add_f32_e32 v6, v5, v5\n"))
    assert (nk, ni, len(rest)) == (1, 3, 1)
    assert set(_build.HAZARD_CHECKED) <= set(_build.SOURCES) and "lattice_wd.hip" in _build.HAZARD_CHECKED
    # every source that holds inline assembly -- in its own code or in a header it includes, directly or through another
    # header; a comment that says "asm" is not code -- is on the list, and no source includes another source
    # (only // comments are dropped, so a /* */ one that says "asm" still counts; includes with a path -- the C ABI header
    # under include/, which has no code -- are not followed)
    import re

    def code(name):
        with open(os.path.join(_build.CSRC, name)) as f:
            return re.sub(r"//[^\n]*", "", f.read())

    def reach(name, seen):
        if name not in seen:
            seen.add(name)
            for inc in re.findall(r'#include "(\w+\.\w+)"', code(name)):
                assert inc.endswith(".h"), (name, inc)
                reach(inc, seen)
        return seen

    for src in _build.SOURCES:
        files = reach(src, set())
        assert files - {src} <= set(_build.HEADERS), (src, files)       # (what the fingerprint and the source rules cover)
        holds = any(re.search(r"\basm\b", code(f)) for f in files)
        assert holds == (src in _build.HAZARD_CHECKED), src


def test_package_self_test_ships_the_golden_data_and_skips_cleanly_without_a_gpu():
    """`python -m warp_rnnt.test` (pytorch_binding/README.md:76-79): the data file inside the package is the repository's
    golden file, byte for byte; on a machine without a GPU every case is skipped (there is no CPU path to fall back to)
    and the command exits 0."""
    with open(os.path.join(ROOT, "warp_rnnt", "golden_vectors.json"), "rb") as f, \
            open(os.path.join(GOLDEN, "reference_vectors.json"), "rb") as g:
        assert f.read() == g.read()
    if torch.cuda.is_available():
        pytest.skip("the GPU suite runs it for real (tests/test_gpu_wrapper.py)")
    out = subprocess.run([sys.executable, "-m", "warp_rnnt.test"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "skipped" in out.stderr and "FAILED" not in out.stderr


def test_rccl_debug_parser_tolerates_whatever_it_is_given():
    """bench.py's first-contact record (n_gpus > 1): RCCL's own NCCL_DEBUG=INFO lines -> version + transport per rank.  The
    parser must never raise and never invent: absent lines, another wording, an empty or missing file give None."""
    import bench
    p = bench.parse_rccl_debug
    assert p(None) == p("") == {"version": None, "channels_via": {}, "transport": None}
    assert p("garbage\n\x00\xff via\nvia \n NCCL version\n")["transport"] is None
    text = ("n1:77:77 [0] NCCL INFO NCCL version 2.22.3+hip7.0\n"
            "n1:77:99 [0] NCCL INFO Channel 00/0 : 0[0] -> 1[1] via P2P/IPC\n"
            "n1:77:99 [0] NCCL INFO Channel 01/0 : 0[0] -> 1[1] via P2P/IPC/read\n"
            "n1:77:99 [0] NCCL INFO Channel 02/0 : 0[0] -> 7[7] via P2P/direct pointer\n")
    r = p(text)
    assert r["version"] == "2.22.3+hip7.0" and r["transport"] == "P2P" and sum(r["channels_via"].values()) == 3
    r = p(text + "n1:77:99 [0] NCCL INFO Channel 00 : 0[0] -> 1[1] via SHM/direct/direct\n")
    assert r["transport"] == "mixed" and r["channels_via"]["SHM"] == 1
    assert p("x NCCL INFO Channel 00/0 : 0[0] -> 1[1] [send] via NET/Socket/0")["transport"] == "NET"
    assert p("RCCL version : 2.21.5-HEAD:abc")["version"].startswith("2.21.5")


def test_lazy_log_softmax_handle_computes_nothing_until_somebody_looks(monkeypatch):
    """warp_rnnt_amd.functional: the handle's mechanics on the CPU (the kernels behind it stubbed with torch's): no compute
    at construction, one materialisation for any number of consumers, autograd through both the handle and its logits,
    and what makes a handle fusable."""
    from warp_rnnt_amd import functional as F2
    calls = {"fwd": 0, "bwd": 0}

    def fake_fwd(x, out=None):
        calls["fwd"] += 1
        return torch.log_softmax(x, -1)

    def fake_bwd(g, y, grad_in=None):
        calls["bwd"] += 1
        return g - torch.exp(y) * g.sum(-1, keepdim=True)
    monkeypatch.setattr(F2.ops, "log_softmax", fake_fwd)
    monkeypatch.setattr(F2.ops, "log_softmax_backward", fake_bwd)
    x = torch.randn(2, 3, 4, 5, requires_grad=True)
    h = F2._LazyLogSoftmaxFn.apply(x)
    h._src = x
    assert isinstance(h, F2.LazyLogSoftmax) and calls == {"fwd": 0, "bwd": 0} and not h.materialised
    assert h.shape == x.shape and h.dtype == x.dtype and h.requires_grad and h.grad_fn is not None and h.fusable()
    assert "materialised=False" in repr(h) and calls["fwd"] == 0
    s1, s2 = (h * 2).sum(), h[0].sum()                          # two consumers, one materialisation
    assert calls["fwd"] == 1 and h.materialised
    (s1 + s2).backward()
    x2 = x.detach().clone().requires_grad_(True)
    lp = torch.log_softmax(x2, -1)
    ((lp * 2).sum() + lp[0].sum()).backward()
    assert torch.allclose(x.grad, x2.grad, atol=1e-6) and calls["bwd"] >= 1
    leaf = F2._LazyLogSoftmaxFn.apply(torch.randn(2, 3, 4, 5))
    leaf._src = torch.zeros(())
    assert leaf.fusable() and not leaf.requires_grad
    leaf.requires_grad_(True)
    assert not leaf.fusable()                                    # d/d log-probs is wanted: the ordinary path
    m = leaf.materialise()
    assert type(m) is torch.Tensor and m.grad_fn is not None
    assert not F2._LazyLogSoftmaxFn.apply(torch.randn(6, 5)).fusable()      # not (N,T,U,V)
    with pytest.raises(RuntimeError, match="fp32 tensor on the GPU"):
        F2.log_softmax(torch.randn(2, 3))
