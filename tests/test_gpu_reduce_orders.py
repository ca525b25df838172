"""biahub_amd/csrc/reduce.hpp is held to the orders its header comment states: tests/reduce_probe.hip (a stand-alone program that
includes only that header) runs every helper in one workgroup, and its results are compared, bit for bit, with a numpy emulation
written from the comment's one-line statements:

  wave_reduce     for d = 32, 16, 8, 4, 2, 1: v = op(v, v of lane ^ d); every lane the same bits
  wave_totals     red[w] = wave_reduce of wave w
  block_reduce    op(op(op(red[0], red[1]), red[2]), red[3]) on thread 0
  block_reduce_n  the same per value, column k folded by thread k
  tree_reduce     red[t] = v; for o = NT/2 .. 1: red[t] = op(red[t], red[t + o]) for t < o; red[0] to every thread
"""

import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
THREADS = {0: 64, 1: 256, 2: 256, 3: 256, 4: 256, 5: 256, 6: 1024, 7: 256}
F32, F64, I32, U64, FM32, FM64 = range(6)
PAIR = {FM32: np.dtype([("v", "<f4"), ("i", "<i8")], align=True), FM64: np.dtype([("v", "<f8"), ("i", "<i8")], align=True)}
DTYPE = {F32: np.dtype("<f4"), F64: np.dtype("<f8"), I32: np.dtype("<i4"), U64: np.dtype("<u8"), **PAIR}
SUM, MIN, MAX, FIRST = range(4)


def first_max(a, b):
    take = (b["v"] > a["v"]) | ((b["v"] == a["v"]) & (b["i"] < a["i"]))
    return np.where(take, b, a)


OPS = {SUM: lambda a, b: a + b, MIN: np.fmin, MAX: np.fmax, FIRST: first_max}  # fmin / fmax: a NaN operand is ignored


# ------------------------------------------------------------------------------------------------ the orders, from the comment
def wave_reduce(v, op):
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = op(v, v[lane ^ d])
    return v


def wave_totals(v, op):
    return np.concatenate([wave_reduce(v[64 * w: 64 * w + 64], op)[:1] for w in range(len(v) // 64)])


def fold_left(red, op):
    r = red[:1]
    for w in range(1, len(red)):
        r = op(r, red[w: w + 1])
    return r


def block_reduce(v, op):
    return fold_left(wave_totals(v, op), op)


def tree_reduce(v, op):
    red = v.copy()
    o = len(red) // 2
    while o > 0:
        red[:o] = op(red[:o], red[o: 2 * o])
        o //= 2
    return red[:1]


def pairwise_waves(v, op):  # not one of the header's orders: the explicit combine of the one-pass deskew's mean
    red = wave_totals(v, op)
    return op(op(red[0:1], red[1:2]), op(red[2:3], red[3:4]))


def serial(v, op):
    return fold_left(v, op)


def expected(helper, v, op):
    if helper == 0:
        return wave_reduce(v, op)
    if helper == 1:
        return wave_totals(v, op)
    if helper == 2:
        return block_reduce(v, op)
    if helper in (3, 7):
        f = block_reduce if helper == 3 else tree_reduce
        return np.concatenate([f(v[:256], op), f(v[256:], op)])
    if helper == 4:
        return np.concatenate([block_reduce(v[256 * k: 256 * k + 256], op) for k in range(3)])
    r = tree_reduce(v, op)
    return np.concatenate([r, r])


def spread(rng, n):
    """normal * 2**k, k uniform in [-20, 20): sums whose bits depend on the order"""
    return rng.standard_normal(n) * 2.0 ** rng.uniform(-20, 20, n)


def hexes(a):
    if a.dtype.names:
        w = "%08x" if a.dtype["v"].itemsize == 4 else "%016x"
        u = a["v"].view("<u4" if a.dtype["v"].itemsize == 4 else "<u8")
        return [(w % int(x)) + ":" + str(int(i)) for x, i in zip(u, a["i"])]
    u = a.view({4: "<u4", 8: "<u8"}[a.dtype.itemsize])
    return [("%08x" if a.dtype.itemsize == 4 else "%016x") % int(x) for x in u]


# ------------------------------------------------------------------------------------------------------------------ the cases
def pairs(kind, v, idx=None):
    a = np.zeros(len(v), PAIR[kind])
    a["v"] = v
    a["i"] = np.arange(len(v)) * 97 % len(v) if idx is None else idx  # a bijection: the smaller index is not the earlier thread
    return a


def build_cases():
    """name -> list of (helper, type, op, values)"""
    rng = np.random.default_rng(0)
    cases = {}
    spread64 = np.concatenate([spread(rng, 256), spread(rng, 768)])  # the first 256: seed 0's first draws, the workgroup cases
    for kind, name in ((F64, "f64"), (F32, "f32")):
        dt = DTYPE[kind]
        x = spread64.astype(dt)
        cases[f"orders_{name}"] = [(0, kind, SUM, x[:64]), (1, kind, SUM, x[:256]), (2, kind, SUM, x[:256]), (4, kind, SUM, x[:768]),
                                   (5, kind, SUM, x[:256]), (6, kind, SUM, x)]
        # the looped variants fold twice into the same red, different data each time
        cases[f"reused_lds_{name}"] = [(3, kind, SUM, x[256:768]), (7, kind, SUM, x[256:768]), (3, kind, MAX, x[:512]), (7, kind, MIN, x[:512])]
        ident = {SUM: dt.type(0), MIN: dt.type(np.inf), MAX: dt.type(-np.inf)}
        few = []
        for op in (SUM, MIN, MAX):
            for nvalues in (10, 0):  # fewer values than a wavefront, and none: the other threads hold the identity
                for helper in (0, 2, 5, 6):
                    v = np.full(THREADS[helper], ident[op], dt)
                    v[:nvalues] = x[:nvalues]
                    few.append((helper, kind, op, v))
        cases[f"few_and_none_{name}"] = few
        nan = []
        for op in (MIN, MAX):
            for helper in (0, 1, 2, 5, 6):
                v = x[: THREADS[helper]].copy()
                v[rng.random(len(v)) < 0.25] = np.nan  # a NaN among the operands is ignored
                v[::64][np.isnan(v[::64])] = 1.0  # wave_totals prints every wave's total: each wave keeps a number
                nan.append((helper, kind, op, v))
                v = np.full(THREADS[helper], np.nan, dt)  # all NaN but one thread, which holds the identity: the identity
                v[len(v) // 3] = ident[op]
                if helper != 1:
                    nan.append((helper, kind, op, v))
        cases[f"nan_ignored_{name}"] = nan
    for kind, name in ((FM64, "f64"), (FM32, "f32")):
        vt = PAIR[kind]["v"].type
        ties = []
        for where in ((69, 101), (10, 200), (0, 255)):  # two lanes of one wavefront, two wavefronts, first and last thread
            for swap in (False, True):
                v = rng.random(1024).astype(vt)
                idx = np.arange(1024) * 97 % 1024
                if swap:  # the tie's smaller index on the later thread
                    idx[[where[0], where[1]]] = idx[[where[1], where[0]]]
                v[list(where)] = 2.0
                ties += [(2, kind, FIRST, pairs(kind, v[:256], idx[:256])), (5, kind, FIRST, pairs(kind, v[:256], idx[:256])),
                         (6, kind, FIRST, pairs(kind, v, idx))]
        v = rng.random(64).astype(vt)
        v[[5, 37]] = 2.0
        ties.append((0, kind, FIRST, pairs(kind, v)))
        for fillv in (1.0, -np.inf):  # all equal, and -inf everywhere: the smallest index
            for helper in (0, 2, 5, 6):
                ties.append((helper, kind, FIRST, pairs(kind, np.full(THREADS[helper], fillv, vt))))
        empty = pairs(kind, np.full(256, -np.inf, vt), np.full(256, 256))  # no thread saw a value: the identity {-inf, n}
        ties += [(2, kind, FIRST, empty), (5, kind, FIRST, empty)]
        cases[f"first_max_ties_{name}"] = ties
    big = (np.uint64(1) << np.uint64(53)) + rng.integers(1, 1 << 20, 1024).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    ints = rng.integers(-(1 << 20), 1 << 20, 1024).astype(np.int32)
    cases["integers"] = [(h, U64, SUM, big[: n]) for h, n in ((0, 64), (1, 256), (2, 256), (3, 512), (4, 768), (5, 256), (6, 1024), (7, 512))]
    cases["integers"] += [(h, I32, op, ints[: THREADS[h]]) for h in (0, 2, 5, 6) for op in (SUM, MIN, MAX)]
    return cases


CASES = build_cases()


def compile_probe(exe):
    from biahub_amd.build import ARCH, CSRC, _hipcc

    cmd = [_hipcc(), "-O2", f"--offload-arch={ARCH}", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", str(ROOT / "tests" / "reduce_probe.hip"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def probe_lines(tmp_path_factory, gpu):
    d = tmp_path_factory.mktemp("reduce_probe")
    compile_probe(d / "reduce_probe")
    with open(d / "records.bin", "wb") as f:
        for name in sorted(CASES):
            for helper, kind, op, v in CASES[name]:
                assert v.dtype == DTYPE[kind]
                f.write(struct.pack("<4i", helper, kind, op, len(v)))
                f.write(np.ascontiguousarray(v).tobytes())
    r = subprocess.run([str(d / "reduce_probe"), str(d / "records.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [int(w[0]) for w in lines] == list(range(sum(len(c) for c in CASES.values())))
    return [w[1:] for w in lines]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_header_keeps_its_stated_orders(probe_lines, name):
    first = sum(len(CASES[n]) for n in sorted(CASES) if n < name)
    for k, (helper, kind, op, v) in enumerate(CASES[name]):
        want = hexes(expected(helper, v, OPS[op]))
        got = probe_lines[first + k]
        print(name, "helper", helper, "op", op, "got", got[:4], "want", want[:4])
        assert got == want, (name, k, helper, op)


def test_the_inputs_tell_the_orders_apart():
    """Before the comparison above is trusted: on the float64 order inputs the butterfly with the left-to-right combine, the
    pairwise wave combine, the tree and the serial sum are four different bit patterns, so a wrong order cannot pass."""
    for name in ("orders_f64", "orders_f32"):
        v = next(x for h, _, _, x in CASES[name] if h == 2)
        got = {f.__name__: hexes(f(v, OPS[SUM]))[0] for f in (block_reduce, pairwise_waves, tree_reduce, serial)}
        assert len(set(got.values())) == 4, got
    few = [c for c in CASES["few_and_none_f64"] if c[0] == 2 and c[2] == MIN]
    assert [hexes(block_reduce(v, OPS[MIN]))[0] for _, _, _, v in few][1] == "7ff0000000000000"  # none: the identity


def test_ties_are_won_by_the_smaller_index():
    """The emulation itself: every first_max tie case names the smallest index among the maxima, wherever it sits."""
    for name in ("first_max_ties_f64", "first_max_ties_f32"):
        for helper, _, _, v in CASES[name]:
            want = v["i"][v["v"] == v["v"].max()].min()
            assert all(int(h.split(":")[1]) == want for h in hexes(expected(helper, v, first_max)))


def test_probe_cross_compiles(tmp_path):
    """reduce.hpp is self-contained: the probe includes nothing else of the project and builds for gfx950 without a GPU."""
    compile_probe(tmp_path / "reduce_probe")
    text = (ROOT / "tests" / "reduce_probe.hip").read_text()
    assert [ln for ln in text.splitlines() if ln.startswith('#include "')] == ['#include "reduce.hpp"']
    header = (ROOT / "biahub_amd" / "csrc" / "reduce.hpp").read_text()
    assert [ln for ln in header.splitlines() if ln.startswith("#include")] == ["#include <hip/hip_runtime.h>"]
