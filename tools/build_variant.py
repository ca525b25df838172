#!/usr/bin/env python3
"""Build a tuning variant of libbhcore.so: `tools/build_variant.py NAME -DBH_FC_XNT=512 ...` compiles translation units of csrc with the
extra flags and links them with the stock objects into biahub_amd/build/variants/libbhcore_NAME.so (A/B runs on one GPU box:
BHCORE_LIB=<that file> python bench.py ...).  Default: the whole FFT engine (fftconv.hip and its four kernel families), so that a
constant several of them read (BH_FC_NT, BH_FC_XNT, BH_FC_PK_CMUL) reaches every user.  `--src=A.hip[,B.hip...]` as the first flag names
the units instead: one family for a switch only it reads (--src=fftconv_colreg.hip -DBH_COLZ_PKROT=0), or another file (--src=affine.hip)."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from biahub_amd import build as B  # noqa: E402

name, flags = sys.argv[1], sys.argv[2:]
srcs = ["fftconv.hip", "fftconv_col.hip", "fftconv_xtile.hip", "fftconv_xw.hip", "fftconv_colreg.hip"]
if flags and flags[0].startswith("--src="):
    srcs, flags = flags[0][6:].split(","), flags[1:]
B.build(verbose=False)
out = B.PKG / "build" / "variants"
out.mkdir(parents=True, exist_ok=True)
base = ["-O3", f"--offload-arch={B.ARCH}", "-fPIC", "-std=c++17", f"-I{B.INCLUDE}", f"-I{B.CSRC}", "-Wall", "-Wno-unused-function"]
variant = {src: out / f"{src.split('.')[0]}_{name}.o" for src in srcs}
procs = [subprocess.Popen([B._hipcc(), *base, *flags, "-c", str(B.CSRC / src), "-o", str(obj)]) for src, obj in variant.items()]
if any(p.wait() for p in procs):
    sys.exit("a variant unit failed to compile")
objs = [str(variant.get(s, B.PKG / "build" / (s + ".o"))) for s in B.SOURCES]
lib = out / f"libbhcore_{name}.so"
subprocess.run([B._hipcc(), f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", str(lib), *objs, "-L/opt/rocm/lib", "-lhipfft",
                "-Wl,-rpath,/opt/rocm/lib"], check=True)
print(lib)
