"""csrc/orca_lds.h: the one description of the ORCA kernels' dynamic LDS that both the kernels (region offsets) and the host (launch
bytes) read.  A small g++ program prints every layout of the sweep; the totals must equal the host formulas orca_plan /
orca_robot_launch used before the header existed (restated below from that arithmetic), and the regions must be aligned for their
element type, disjoint and gap-free up to the total.

The restated formulas were checked against the originals: the four C++ expressions were copied verbatim from the previous orca.hip
into a stand-alone program (sizeof(float4) = 16, sizeof(float2) = 8) and agreed with these Python functions on the whole sweep."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "social_navigation_pyenvs_amd", "csrc")

ROWS = [1, 2, 5, 25, 26, 32, 33, 64, 65, 256, 257, 512]
KS = [0, 1, 5, 10, 16]
KOS = [0, 1, 16]
ROBOT_N = [1, 5, 63, 127]
F4, F2, F1 = 16, 8, 4

PROGRAM = r"""
#include <cstdio>
#include "orca_lds.h"
using namespace csimpl;
#define R(n, e) std::printf(" " #n ":%u:%u:%d", o.n.off, o.n.bytes, e)
int main(int argc, char** argv)
{
    int v[8] = {0};
    for (int line = 0; std::scanf("%d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]) == 7; ++line) {
        if (argv[1][0] == 's') { const OrcaStepLds o = orca_step_lds(v[0], v[1], v[2], v[3], v[4], v[5], v[6]); std::printf("%u", o.total);
            R(pv, 16); R(L, 16); R(P, 16); R(rowP, 16); R(rowA, 8); R(q, 16); R(r, 4); R(nd, 4); R(ni, 4); R(rp, 4); R(g0x, 4); R(flag, 4); R(od, 4); R(oi, 4); R(sel, 4); }
        if (argv[1][0] == 'r') { const OrcaRobotLds o = orca_robot_lds(v[0], v[1]); std::printf("%u", o.total); R(L, 16); R(P, 16); R(nd, 4); R(ni, 4); R(od, 4); R(oi, 4); }
        if (argv[1][0] == 'f') { const OrcaRobotFastLds o = orca_robot_fast_lds(v[0], v[1]); std::printf("%u", o.total); R(pv, 16); R(rr, 4); R(ln, 16); R(pr, 16); R(pa, 8); R(q, 16); R(sel, 4); }
        if (argv[1][0] == 'g') { const OrcaGridLds o = orca_grid_lds(v[0], v[1], v[2]); std::printf("%u", o.total); R(ln, 16); R(pr, 16); R(pa, 8); R(q, 16); R(sel, 4); R(nd, 4); R(ni, 4); R(od, 4); R(oi, 4); }
        std::printf("\n");
    }
    return 0;
}
"""


# ---- the host formulas as orca_plan / orca_robot_launch wrote them out by hand ------------------------------------------------
def old_block_shmem(fast10, lp3_static, T, TL, K, KO):
    fixed = T * (2 * F4 + 4 * F1)
    if fast10:
        return fixed + 10 * TL * F4 + (0 if lp3_static else 72 * (F4 + F2)) + T * (F4 + F1)
    return fixed + (K + KO) * TL * (2 * F4 + 2 * F1)


def old_grid_shmem(fast10, K, KO):
    if fast10:
        return (10 * 64 + 72 + 64) * F4 + 72 * F2 + 64 * F1
    return (K + KO) * 64 * (2 * F4) + (K + KO) * 64 * (F1 + F1)


def old_robot_shmem(K, KO):
    return (K + KO) * 64 * (2 * F4 + 2 * F1)


def old_robot_fast_shmem(wpb, n):
    return wpb * (n + 1) * F4 + ((wpb * (n + 1) + 3) & ~3) * F1 + (10 + 1) * 64 * F4 + 72 * (F4 + F2) + 64 * F1


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    d = tmp_path_factory.mktemp("orca_lds")
    src, exe = d / "lds.cpp", d / "lds"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(kind, configs):
        text = "".join(" ".join(str(int(x)) for x in (list(c) + [0] * 7)[:7]) + "\n" for c in configs)
        out = subprocess.run([str(exe), kind], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(configs)
        res = []
        for ln in out:
            f = ln.split()
            res.append((int(f[0]), [(n, int(o), int(b), int(e)) for n, o, b, e in (x.split(":") for x in f[1:])]))
        return res

    return run


def check_regions(total, regions, what):
    end = 0
    for name, off, nbytes, elem in regions:   # declared in layout order: aligned, back to back, none overlapping
        assert off % elem == 0, (what, name, off, elem)
        assert nbytes % elem == 0, (what, name, nbytes, elem)
        assert off == end, (what, name, off, end)
        end = off + nbytes
    assert end == total, (what, end, total)


def block_configs():
    out = []
    for rows in ROWS:
        T = 64 if rows <= 64 else (256 if rows <= 256 else 512)
        wpb = 64 // rows if rows <= 64 else 1
        for lp3_static in (0, 1):
            out.append((1, lp3_static, T, wpb, rows, 10, 0))   # the register-resident build: maxNeighbors = 10, no obstacle lines
            for K in KS:
                for KO in KOS:
                    out.append((0, lp3_static, T, wpb, rows, K, KO))
    return out


def test_step_kernel_layout_matches_the_host_formula(layouts):
    cfgs = block_configs()
    for c, (total, regions) in zip(cfgs, layouts("s", cfgs)):
        fast10, lp3_static, T, wpb, rows, K, KO = c
        assert total == old_block_shmem(fast10, lp3_static, T, wpb * rows, K, KO), c
        check_regions(total, regions, c)


def test_grid_kernel_layout_matches_the_host_formula(layouts):
    cfgs = [(1, 10, 0)] + [(0, K, KO) for K in KS for KO in KOS]
    for c, (total, regions) in zip(cfgs, layouts("g", cfgs)):
        assert total == old_grid_shmem(*c), c
        check_regions(total, regions, c)


def test_robot_kernel_layouts_match_the_host_formulas(layouts):
    cfgs = [(K, KO) for K in KS for KO in KOS]
    for c, (total, regions) in zip(cfgs, layouts("r", cfgs)):
        assert total == old_robot_shmem(*c), c
        check_regions(total, regions, c)
    cfgs = [(16, n) for n in ROBOT_N]
    for c, (total, regions) in zip(cfgs, layouts("f", cfgs)):
        assert total == old_robot_fast_shmem(*c), c
        check_regions(total, regions, c)
