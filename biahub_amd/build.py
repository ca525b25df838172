"""Build libbhcore.so (HIP, gfx950) in-tree with hipcc.  `python -m biahub_amd.build`."""

from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
INCLUDE = PKG.parent / "include"
LIB = PKG / "libbhcore.so"
# longest compiles first (the pool below starts sources in this order): pyramid.hip alone takes longer than any other file, then
# the kernel families of the FFT engine
SOURCES = ["pyramid.hip", "fftconv_col.hip", "fftconv_xtile.hip", "fftconv_xw.hip", "fftconv_colreg.hip", "deskew.hip", "stitch.hip", "stitch_pcc.hip", "focus.hip", "affine.hip", "fftconv.hip", "context.hip", "fill.hip", "deconv.hip", "spline.hip", "copy.hip", "regmetric.hip", "moments.hip", "graphmatch.hip", "flatfield.hip", "psffit.hip", "stackreg.hip", "psf.hip", "binning.hip", "codec.hip", "lz4.hip", "zstd.hip", "zstd_enc.hip", "mask.hip", "invtf.hip", "host_deskew.hip"]
ARCH = "gfx950"


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


# textual includes of a translation unit (rebuild triggers)
_FC = ("fftconv.hpp", "fftconv_dev.hpp")
INCLUDES = {"fftconv.hip": _FC + ("tune_rule.hpp",), "fftconv_col.hip": _FC, "fftconv_xtile.hip": _FC + ("fftconv_xpass.inc",), "fftconv_xw.hip": _FC + ("fftconv_regfft.inc", "fftconv_xrows.inc", "fftconv_xw.inc", "fftconv_x3.inc"),
            "fftconv_colreg.hip": _FC + ("fftconv_regfft.inc", "fftconv_colw.inc", "fftconv_colz.inc", "fftconv_colz3.inc", "fftconv_zdirect.inc"),
            "deconv.hip": ("fftconv.hpp",), "invtf.hip": ("fftconv.hpp",), "affine.hip": ("affine_zwalk.inc", "affine_zoblique.inc"),
            "deskew.hip": ("deskew_geom.hpp", "deskew_rows.inc"), "host_deskew.hip": ("deskew_geom.hpp",), "lz4.hip": ("blosc_frame.hpp",),
            "zstd.hip": ("zstd_lanes.inc", "zstd_format.inc", "zstd_frame.inc", "zstd_block.inc", "blosc_frame.hpp"),
            "zstd_enc.hip": ("zstd_lanes.inc", "zstd_format.inc", "zstd_enc.inc", "blosc_frame.hpp")}


def needs_build() -> bool:
    if not LIB.exists():
        return True
    t = LIB.stat().st_mtime
    deps = [CSRC / s for s in SOURCES] + [CSRC / "common.hpp", CSRC / "reduce.hpp", INCLUDE / "bhcore.h"] + [CSRC / i for v in INCLUDES.values() for i in v]
    return any(d.stat().st_mtime > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> Path:
    if not force and not needs_build():
        return LIB
    objdir = PKG / "build"
    objdir.mkdir(exist_ok=True)
    flags = ["-O3", f"--offload-arch={ARCH}", "-fPIC", "-std=c++17", f"-I{INCLUDE}", f"-I{CSRC}",
             "-Wall", "-Wno-unused-function"]

    def compile_one(src: str) -> Path:
        obj = objdir / (src + ".o")
        srcp = CSRC / src
        hdr_t = max([(CSRC / "common.hpp").stat().st_mtime, (CSRC / "reduce.hpp").stat().st_mtime, (INCLUDE / "bhcore.h").stat().st_mtime]
                    + [(CSRC / i).stat().st_mtime for i in INCLUDES.get(src, ())])
        if not force and obj.exists() and obj.stat().st_mtime > max(srcp.stat().st_mtime, hdr_t):
            return obj
        cmd = [_hipcc(), *flags, "-c", str(srcp), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(LIB), *map(str, objs),
           "-L/opt/rocm/lib", "-lhipfft", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
