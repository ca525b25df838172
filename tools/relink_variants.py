#!/usr/bin/env python3
"""Relink every tuning variant under biahub_amd/build/variants against the CURRENT stock objects (after the other translation
units changed): `tools/relink_variants.py`.  A variant object is `<unit>_<name>.o` (tools/build_variant.py); a variant may have several."""
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from biahub_amd import build as B  # noqa: E402

B.build(verbose=False)
out = B.PKG / "build" / "variants"
variants = {}  # name -> {source: object}
for obj in sorted(out.glob("*.o")):
    # the unit is the longest source stem the object's name starts with (fftconv_xw_NAME.o belongs to fftconv_xw.hip, not fftconv.hip)
    src = max((s for s in B.SOURCES if obj.stem.startswith(s[:-4] + "_")), key=len, default=None)
    if src is None:
        print(f"skipped {obj.name}: no current translation unit has that stem")
        continue
    variants.setdefault(obj.stem[len(src) - 3:], {})[src] = obj
for name, variant in variants.items():
    objs = [str(variant.get(s, B.PKG / "build" / (s + ".o"))) for s in B.SOURCES]
    lib = out / f"libbhcore_{name}.so"
    subprocess.run([B._hipcc(), f"--offload-arch={B.ARCH}", "-shared", "-fPIC", "-o", str(lib), *objs, "-L/opt/rocm/lib", "-lhipfft",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    print(lib.name)
