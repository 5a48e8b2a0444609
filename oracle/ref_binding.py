"""Recipe for oracle/_ref/_C_ref.so: the reference's own pytorch_binding/binding.cpp, linked whole against
include/warp_rnnt_amd.h + libwarp_rnnt_amd.so -- TEST INFRASTRUCTURE ONLY.

``build()`` (__graft_entry__.build) runs this where a checkout of the reference lies at ``REFERENCE``
(``$RNNT_REFERENCE_DIR`` overrides): the file is read where it lies, edited in memory, written to oracle/_ref/ and
compiled there with every symbol required to resolve (-Wl,--no-undefined).  oracle/_ref/ is a build product and
stays out of git; tests/test_host_cpu.py loads the module from it and skips when no reference was there to build
it from.  Nothing of the reference is kept in the repository."""
import os
import shutil
import subprocess
import sys
import sysconfig

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
REFERENCE = os.environ.get("RNNT_REFERENCE_DIR", "/root/reference")
OUT_DIR = os.path.join(_HERE, "_ref")
MODULE = os.path.join(OUT_DIR, "_C_ref.so")
SOURCE = os.path.join(OUT_DIR, "binding_ref_edited.cpp")

# What a maintainer of the reference changes in pytorch_binding/binding.cpp.  The first edit is the header; the rest
# is what PyTorch-ROCm's own hipify pass does to every extension source (CUDA c10 names -> their "masquerading" HIP
# twins), written out so that the recipe does not depend on that tool.
EDITS = [
    ('#include "core.h"', '#include "warp_rnnt_amd.h"'),
    ("#include <c10/cuda/CUDAGuard.h>", "#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>"),
    ("#include <c10/cuda/CUDAStream.h>", "#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>"),
    ("c10::cuda::getCurrentCUDAStream(", "c10::hip::getCurrentHIPStreamMasqueradingAsCUDA("),
    ("at::cuda::OptionalCUDAGuard", "c10::hip::OptionalHIPGuardMasqueradingAsCUDA"),
]
# the five core.h entry points the binding calls
ENTRY_POINTS = ("run_warp_rnnt(", "run_warp_rnnt_gather(", "run_gather_for_compact(", "run_warp_rnnt_compact(",
                "run_scatter_grad_for_compact(")


def reference_binding():
    return os.path.join(REFERENCE, "pytorch_binding", "binding.cpp")


def build(lib, verbose=False):
    """Compile the edited reference binding against `lib` (the path of libwarp_rnnt_amd.so).  Returns the module's
    path, or None when no reference checkout is readable here (an existing module is then left as it is)."""
    src_path = reference_binding()
    if not os.access(src_path, os.R_OK):
        return None
    deps = [src_path, lib, os.path.join(ROOT, "include", "warp_rnnt_amd.h"), os.path.abspath(__file__)]
    if os.path.exists(MODULE) and all(os.path.getmtime(MODULE) >= os.path.getmtime(d) for d in deps):
        return MODULE
    import torch
    from torch.utils import cpp_extension as ce
    gxx = shutil.which(os.environ.get("CXX", "g++"))
    if gxx is None:
        raise RuntimeError("no g++ to build the reference binding with")
    text = open(src_path).read()
    for old, new in EDITS:
        if old not in text:
            raise RuntimeError(f"the reference's binding.cpp no longer contains {old!r}")
        text = text.replace(old, new)
    for name in ENTRY_POINTS:
        if name not in text:
            raise RuntimeError(f"the reference's binding.cpp no longer calls {name!r}")
    os.makedirs(OUT_DIR, exist_ok=True)
    with open(SOURCE, "w") as f:
        f.write(text)
    tdir = os.path.dirname(torch.__file__)
    tmp = MODULE + ".tmp"
    cmd = [gxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-DTORCH_EXTENSION_NAME=_C_ref", "-DTORCH_API_INCLUDE_EXTENSION_H",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI),
           "-I" + os.path.join(ROOT, "include")]
    cmd += ["-I" + p for p in ce.include_paths(device_type="cuda")] + ["-I" + sysconfig.get_paths()["include"]]
    # (the library is found next to the tree the module lies in, wherever that tree is copied to)
    rel = os.path.relpath(os.path.dirname(os.path.abspath(lib)), OUT_DIR)
    cmd += [SOURCE, "-o", tmp, "-Wl,--no-undefined", "-L" + os.path.join(tdir, "lib"),
            "-L" + os.path.dirname(lib), "-lwarp_rnnt_amd", "-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch_hip",
            "-ltorch", "-ltorch_python", "-lamdhip64",
            "-L" + sysconfig.get_config_var("LIBDIR"), "-lpython" + sysconfig.get_config_var("LDVERSION"),
            "-Wl,-rpath,$ORIGIN/" + rel, "-Wl,-rpath," + os.path.join(tdir, "lib")]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    if res.returncode != 0:
        raise RuntimeError("building the reference binding failed:\n" + res.stdout.decode()[-6000:])
    os.replace(tmp, MODULE)
    if verbose:
        print("built", MODULE, file=sys.stderr)
    return MODULE
