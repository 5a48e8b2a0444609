"""Diagnostics and A/B knobs -- nothing here is needed in use and nothing in the product calls it.

One arithmetic serves every call (the reference's fp32 log-sum-exp per cell); several kernels implement it with the same
instructions on the chain and the same bits, and the library picks one by shape.  `set_lattice_kernel` pins one for tests
and timing runs (process-wide: `rnnt_amd_debug_set_lattice_kernel`, one atomic int; initial value from the environment
variable RNNT_DEBUG_LATTICE_KERNEL = ws | wd | wl)."""
import collections
import contextlib

from ._lib import load

LATTICE_KERNEL_PINS = ("auto", "ws", "wd", "wl")
LATTICE_KERNELS = ("none", "lattice_ws", "lattice_wd", "(retired)", "lattice (single role)", "lattice_wl")


def set_lattice_kernel(kernel):
    """``"auto"`` by shape, ``"ws"`` compute + I/O wave pairs in one workgroup per sweep, ``"wd"`` one three-wave
    workgroup per 64-column block (boundary columns through L2), ``"wl"`` the same teams in one workgroup per sweep
    wherever it fits.  Same bits whichever runs.  Returns the previous pin."""
    if kernel not in LATTICE_KERNEL_PINS:
        raise ValueError(f"unknown lattice kernel {kernel!r}: expected one of {LATTICE_KERNEL_PINS}")
    return LATTICE_KERNEL_PINS[load().rnnt_amd_debug_set_lattice_kernel(LATTICE_KERNEL_PINS.index(kernel))]


def get_lattice_kernel():
    return LATTICE_KERNEL_PINS[load().rnnt_amd_debug_get_lattice_kernel()]


@contextlib.contextmanager
def lattice_kernel(kernel):
    """``with debug.lattice_kernel("ws"): ...`` -- the pin inside the block, the old one after it (process-wide)."""
    old = set_lattice_kernel(kernel)
    try:
        yield
    finally:
        set_lattice_kernel(old)


def last_lattice_kernel():
    """Name of the lattice kernel this thread's last loss call launched (``rnnt_amd_debug_last_lattice_kernel``)."""
    return LATTICE_KERNELS[load().rnnt_amd_debug_last_lattice_kernel()]


def last_loss_used_blank_plane():
    """Did this process's last loss call on dense log-probs read the blank column from the plane that
    ``ops.log_softmax`` left beside them (``ops.blank_plane_of``)?  Host-side bookkeeping only: nothing is read back."""
    from . import ops
    return ops._LAST_LOSS_PLANE


LatticePlan = collections.namedtuple("LatticePlan", "kernel block_diagonals rings")
LOADERS = ("skewed", "rowmajor", "dense")


def lattice_plan(N, T, U, loader="skewed", flags=True, rings=True, offs32=False, cus=0, pin=None, folded=True):
    """What the library's planner (csrc/lattice_plan.h) would run for a call with these facts, under this process's knobs
    and without a launch (``rnnt_amd_debug_lattice_plan``): ``kernel`` as `last_lattice_kernel` would name it,
    ``block_diagonals`` of lattice_wd (8 or 16), ``rings``: lattice_wd with flags and rings rather than its plain launch.
    ``cus=0``: 256; ``pin=None``: the current pin."""
    r = load().rnnt_amd_debug_lattice_plan(N, T, U, LOADERS.index(loader), int(flags) | int(rings) << 1 | int(offs32) << 2,
                                           cus, -1 if pin is None else LATTICE_KERNEL_PINS.index(pin), int(folded))
    if r < 0:
        raise ValueError(f"no plan for N={N}, T={T}, U={U}, pin={pin!r}")
    return LatticePlan(LATTICE_KERNELS[r & 255], r >> 8 & 255, bool(r >> 16 & 1))


LSM_MODES = ("norm", "gather", "bwd", "log_softmax_backward")
LSM_DTYPES = ("f32", "bf16", "f16")
LSM_FAMILIES = ("regs", "lgr", "rows", "rows_diag", "small", "large", "generic")
LSM_PLAN_FIELDS = ("family", "KR", "L", "Q", "WP", "TH", "NV", "grid", "grid_y", "grid_z", "lds", "R", "q", "xcd", "head_rows",
                   "tail")


def lsm_plan(mode, dtype, rows, V, T=1, U=1, compact=False, aligned=True, plane=False):
    """What the library's planner (csrc/lsm_plan.h) would launch for a forward log-softmax call with these facts -- ``mode``
    one of `LSM_MODES` (the last: the plan of ``rnnt_amd_log_softmax_backward``), ``dtype`` one of `LSM_DTYPES` -- under this
    process's knobs and without a launch (``rnnt_amd_debug_lsm_plan``).  A dict of `LSM_PLAN_FIELDS`: ``family`` and ``tail``
    (the family behind the register kernel's whole groups, None: nothing left over) by their names in `LSM_FAMILIES`."""
    import ctypes
    out = (ctypes.c_int * len(LSM_PLAN_FIELDS))()
    r = load().rnnt_amd_debug_lsm_plan(LSM_MODES.index(mode), LSM_DTYPES.index(dtype), rows, V, T, U, int(compact),
                                       int(aligned), int(plane), out, len(out))
    if r < 0:
        raise ValueError(f"no plan for rows={rows}, V={V}")
    plan = dict(zip(LSM_PLAN_FIELDS, out))
    plan["family"] = LSM_FAMILIES[plan["family"]]
    plan["tail"] = None if plan["tail"] < 0 else LSM_FAMILIES[plan["tail"]]
    plan["WP"] = bool(plan["WP"])
    return plan
