"""The launch plan of the sampling path (csrc/mst_plan.h) against its Python mirror (tests/plan_mirror.py), on the CPU.

The header is host-only C++: a stand-alone driver (tests/launch_plan_driver.cpp) that includes nothing else of the project is compiled
and run as a child process, and every field of plan_trunk, rows_ntb, plan_slices' count and slice_of's split are compared with the
mirror, for every number of rows from 1 to 260, the frame counts at which a rule changes, guidance on and off, and every switch of the
plan away from its default.  The GPU tests derive their case ids and path tables from the mirror; this is what ties the mirror to the
code the engine runs."""
import os
import shutil
import subprocess

import pytest

import plan_mirror as pm
from conftest import ROOT

CSRC = os.path.join(ROOT, "diffusion-based-motion-style-transfer_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "launch_plan_driver.cpp")

ROWS = range(1, 261)
FRAMES = [1, 5, 16, 17, 20, 60, 76, 100, 150, 191, 192, 196, 207, 208, 223]
KNOB_SETS = {
    "default": {}, "small_m=0": dict(small_m=0), "precise": dict(precise=1),
    "tail_ntb=2": dict(tail_ntb=2), "tail_ntb=3": dict(tail_ntb=3), "tail_ntb=4": dict(tail_ntb=4),
    "nsplit=1": dict(nsplit=1), "nsplit=2": dict(nsplit=2), "nsplit=3": dict(nsplit=3),
    "trunk": dict(trunk_groups=1), "small_ln=0": dict(small_ln=0), "small_fast=0": dict(small_fast=0), "fuse_tail=0": dict(fuse_tail=0),
    "fuse_qkv_attn=0": dict(fuse_qkv_attn=0), "fuse_qkv_attn=2": dict(fuse_qkv_attn=2),
    # the resident trunk beside what vetoes it, and the switches no sweep above moves
    "trunk+small_m=0": dict(trunk_groups=1, small_m=0), "trunk+precise": dict(trunk_groups=1, precise=1),
    "trunk+tail_ntb=4": dict(trunk_groups=1, tail_ntb=4), "trunk+fuse_tail=0": dict(trunk_groups=1, fuse_tail=0),
    "trunk+fuse_qkv_attn=2": dict(trunk_groups=1, fuse_qkv_attn=2), "trunk+9-layers": dict(trunk_groups=1, num_layers=9),
    "trunk+dbg_stop": dict(trunk_groups=1, dbg_stop=1), "trunk+nsplit=3": dict(trunk_groups=1, nsplit=3),
    "dbg_stop": dict(dbg_stop=1), "small_ln_m=1000": dict(small_ln_m=1000), "ln128_min_m=4096": dict(ln128_min_m=4096, small_m=0),
}


def mirror_line(k, rows, T):
    out = []
    for sl in (1, 3):
        for ins in (0, 1):
            p = pm.plan_trunk(k, rows, T, sl, ins)
            out += [p[f] for f in pm.PLAN_FIELDS]
    out.append(pm.rows_ntb(rows * (T + 1)))
    for cfg in (0, 1):
        n = pm.plan_slices(k, rows, cfg, T)
        out.append(n)
        for i in range(n):
            out += pm.slice_of(rows, n, i)
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_mirror_equals_the_header_over_the_sweep(tmp_path):
    exe = str(tmp_path / "launch_plan_driver")
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, DRIVER], check=True)
    assert list(pm.KNOBS) == ["small_m", "small_ln", "small_ln_m", "small_fast", "precise", "fuse_qkv_attn", "fuse_tail", "tail_ntb",
                              "ln128_min_m", "trunk_groups", "num_layers", "nsplit", "dbg_stop"]          # PlanKnobs' order
    cases = [(name, pm.knobs(**over), rows, T) for name, over in KNOB_SETS.items() for T in FRAMES for rows in ROWS]
    text = "".join(" ".join(map(str, [*k.values(), rows, T])) + "\n" for _, k, rows, T in cases)
    r = subprocess.run([exe, str(pm.NTB1_M), str(pm.NTB2_FROM)], input=text, capture_output=True, text=True, check=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) == len(KNOB_SETS) * len(FRAMES) * 260
    seen = set()
    for (name, k, rows, T), line in zip(cases, lines):
        got, want = [int(v) for v in line.split()], mirror_line(k, rows, T)
        assert got == want, f"{name}: rows {rows}, T {T}: header {got} != mirror {want}"
        seen.add((got[0], got[32]))
    # the sweep reaches every path and every rows-GEMM tile height
    assert {p for p, _ in seen} == set(range(len(pm.PATHS))) and {n for _, n in seen} == {1, 2, 4}
