"""In-tree build of every native artifact (gfx950 only, no JIT cache):

  elastic_gpu_agent_amd/_amdsmi<ext>.so   pybind11 → libamd_smi enumeration
  elastic_gpu_agent_amd/libegpu_shim.so   HSA interposer (CU mask + HBM quota)
  elastic_gpu_agent_amd/libegpu_kernels.so  gfx950 HIP verification kernels
  bin/egpu-hook                           OCI prestart hook binary

Run: ``python -m elastic_gpu_agent_amd.native.build`` (hipcc cross-compiles
without a GPU; artifacts land in-tree so they travel with the repo snapshot).
"""
from __future__ import annotations

import os
import subprocess
import sys
import sysconfig

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
REPO = os.path.dirname(PKG)


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _newer(target: str, *sources: str) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(s) <= t for s in sources)


def pybind_includes():
    import pybind11

    return [f"-I{pybind11.get_include()}", f"-I{sysconfig.get_paths()['include']}"]


def build_amdsmi(force=False):
    src = os.path.join(HERE, "amdsmi_binding.cpp")
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    out = os.path.join(PKG, f"_amdsmi{ext}")
    if not force and _newer(out, src):
        return out
    _run(
        ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src]
        + pybind_includes()
        + [f"-I{ROCM}/include", f"-L{ROCM}/lib", "-lamd_smi",
           f"-Wl,-rpath,{ROCM}/lib", "-o", out]
    )
    return out


def build_fastwire(force=False):
    src = os.path.join(HERE, "fastwire.cpp")
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    out = os.path.join(PKG, f"_fastwire{ext}")
    headers = [os.path.join(HERE, h) for h in ("wirecore.h", "idruns.h", "hashmemo.h", "bindfx.h")]
    if not force and _newer(out, src, *headers):
        return out
    _run(
        ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src]
        + pybind_includes()
        + ["-o", out, "-lcrypto"]
    )
    return out


def build_etransport(force=False):
    src = os.path.join(HERE, "etransport.cpp")
    tables = os.path.join(HERE, "hpack_tables.h")
    gen = os.path.join(HERE, "gen_hpack_tables.py")
    if not os.path.exists(tables) or os.path.getmtime(tables) < os.path.getmtime(gen):
        _run([sys.executable, gen])
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    out = os.path.join(PKG, f"_etransport{ext}")
    headers = [os.path.join(HERE, h) for h in ("h2core.h", "h2frame.h")]
    if not force and _newer(out, src, tables, *headers):
        return out
    _run(
        ["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", src]
        + pybind_includes()
        + ["-pthread", "-o", out]
    )
    return out


def build_shim(force=False):
    src = os.path.join(HERE, "egpu_shim.cpp")
    out = os.path.join(PKG, "libegpu_shim.so")
    if not force and _newer(out, src):
        return out
    _run(
        ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-DAMD_INTERNAL_BUILD", src,
         f"-I{ROCM}/include", f"-I{ROCM}/include/hsa", "-o", out]
    )
    return out


def build_kernels(force=False):
    srcs = [os.path.join(HERE, f)
            for f in ("egpu_kernels.hip", "egpu_selftest.hip", "egpu_selftest_mx.hip")]
    hdrs = [os.path.join(HERE, h) for h in ("selftest_ref.h", "selftest_mx_ref.h")]
    out = os.path.join(PKG, "libegpu_kernels.so")
    if not force and _newer(out, *srcs, *hdrs):
        return out
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    _run(
        [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", *srcs,
         "-o", out]
    )
    return out


def build_hook(force=False):
    srcs = [os.path.join(HERE, "egpu_hook.cpp"), os.path.join(HERE, "devfilter.cpp")]
    hdr = os.path.join(HERE, "devfilter.h")
    hdr2 = os.path.join(HERE, "minijson.h")
    os.makedirs(os.path.join(REPO, "bin"), exist_ok=True)
    out = os.path.join(REPO, "bin", "egpu-hook")
    if not force and all(_newer(out, s) for s in srcs + [hdr, hdr2]):
        return out
    _run(["g++", "-O2", "-std=c++17", *srcs, "-o", out])
    return out


def build_all(force=False):
    return {
        "amdsmi": build_amdsmi(force),
        "fastwire": build_fastwire(force),
        "etransport": build_etransport(force),
        "shim": build_shim(force),
        "kernels": build_kernels(force),
        "hook": build_hook(force),
    }


if __name__ == "__main__":
    force = "--force" in sys.argv
    arts = build_all(force)
    for k, v in arts.items():
        print(f"{k}: {v}")
