"""The spectrum audition of Richardson-Lucy (csrc/fftconv.hip ``fftconv_tune_spectrum``, rule in csrc/tune_rule.hpp) changes where
the spectrum lives and nothing else: same bits, no candidate left behind, once per block, again after the workspace was
released.  The allocator and the audition read their switches once per process, so every case is a fresh child process;
``BH_FC_TUNE_MIN_VOXELS=1`` lets the audition run on a volume of 2^24 voxels."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = """
import sys, json, numpy as np, torch
sys.path.insert(0, {root!r})
from biahub_amd.deconvolve import PreparedRichardsonLucy
from biahub_amd.device import alloc_layout, get_context
rng = np.random.default_rng(11)
vol = (rng.random((64, 256, 1024), dtype=np.float32) * 300 + 50)
ax = [np.arange(n) - (n - 1) / 2 for n in (9, 5, 5)]
g = [np.exp(-0.5 * (a / s) ** 2) for a, s in zip(ax, (1.5, 1.0, 1.0))]
psf = (g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]).astype(np.float32)
psf /= psf.sum()
dev = torch.device('cuda', 0)
ctx = get_context(dev)
d = torch.from_numpy(vol).to(dev)
def mark(text):
    torch.cuda.synchronize(dev)
    sys.stderr.write('@@ ' + text + chr(10))
    sys.stderr.flush()
with PreparedRichardsonLucy(psf, vol.shape, dev) as h:
    first = h(d, 3, 1e-6).cpu().numpy()
    lay = alloc_layout()
    mark('first call done')
    second = h(d, 3, 1e-6).cpu().numpy()
    mark('second call done')
    ctx.release_workspace()
    third = h(d, 3, 1e-6).cpu().numpy()
    mark('third call done')
np.save(sys.argv[1], np.stack([first, second, third]))
print(json.dumps(lay))
"""

LAYOUTS = {
    "hipmalloc": {},                             # the 67-MB spectrum is below the 2-GiB threshold: a hipMalloc block
    "shuffled_vmm": {"BH_ALLOC_VMM_MIN_MB": "16"},  # ... a block of 2-MiB chunks mapped in a shuffled order
}


def _run(tmp_path, name, env):
    script = tmp_path / "audition_case.py"
    script.write_text(CHILD.format(root=str(ROOT)))
    f = tmp_path / f"{name}.npy"
    base = {k: v for k, v in os.environ.items() if not k.startswith(("BH_FC_TUNE", "BH_ALLOC_"))}
    r = subprocess.run([sys.executable, str(script), str(f)], capture_output=True, text=True,
                       env={**base, "BH_DEBUG_SCRATCH": "1", "BH_FC_TUNE_MIN_VOXELS": "1", **env})
    assert r.returncode == 0, r.stderr[-2000:]
    # "[bh tune] " lines per section of the child's stderr: before the first mark, between the first and second, ...
    sections, count = [], 0
    for line in r.stderr.splitlines():
        if line.startswith("[bh tune] "):
            count += 1
        elif line.startswith("@@ "):
            sections.append(count)
            count = 0
    assert len(sections) == 3, r.stderr[-2000:]
    return np.load(f), json.loads(r.stdout.strip().splitlines()[-1]), sections


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_audition_changes_placement_only(gpu, tmp_path, layout):
    env = LAYOUTS[layout]
    off, lay_off, lines_off = _run(tmp_path, "off", {**env, "BH_FC_TUNE_ALLOC": "0"})
    on, lay_on, lines_on = _run(tmp_path, "on", {**env, "BH_FC_TUNE_ALLOC": "1"})
    assert lines_off == [0, 0, 0]
    # one audition in the first call, none in the second (the block lives), one again after release_workspace
    assert lines_on == [1, 0, 1]
    assert lay_on["shuffled"] == lay_off["shuffled"] and lay_on["chunk_kib"] == lay_off["chunk_kib"]
    if layout == "shuffled_vmm":
        assert lay_off["live_blocks"] >= 1  # the spectrum is a block of mapped chunks here
    # no candidate leaked: the allocator holds what it holds without the audition
    assert lay_on["live_blocks"] == lay_off["live_blocks"] and lay_on["live_gb"] == lay_off["live_gb"]
    assert np.isfinite(off).all() and off[0].std() > 0
    assert np.array_equal(off[0], off[1]) and np.array_equal(off[0], off[2])
    assert np.array_equal(on, off)  # bit-identical, all three calls
