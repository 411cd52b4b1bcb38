"""The arena planner (csrc/device/arena.hpp) without a GPU and without HIP: tests/host_harness/arena_check.cpp includes that header alone (plain g++, no HIP include path),
plans the alignment scratch as ctx.hip's alignment_enqueue does, and prints the offsets; they must be those of the hand-written formula
the planner replaced, restated below."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_BLOCK = 256  # kernels.hpp
INFO_ROW = 88  # sizeof(MomentRow<kAlignInfoTerms>): a count, padding, ten doubles (88 bytes per block, ctx.hpp)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("arena") / "arena_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(REPO, "tests", "host_harness", "arena_check.cpp"), "-o", out], check=True)
    return out


def formula(ns, nt):
    """ctx.hip before the planner: nine offsets and the total"""
    def up(b):
        return (b + 255) & ~255
    nt16 = (nt + 15) & ~15
    nblk = (ns + K_BLOCK - 1) // K_BLOCK
    o_idx = 0
    o_corr = o_idx + up(4 * ns)
    o_d2 = o_corr + up(4 * ns)
    o_inl = o_d2 + up(4 * ns)
    o_hit = o_inl + up(ns)
    o_part = o_hit + up(nt16)
    o_sum = o_part + up(8 * nblk)
    o_rows = o_sum + 256
    o_info = o_rows + up(INFO_ROW * nblk)
    total = o_info + 256
    return [o_idx, o_corr, o_d2, o_inl, o_hit, o_part, o_sum, o_rows, o_info, total]


@pytest.mark.parametrize("ns,nt", [(1, 1), (255, 15), (256, 16), (257, 17), (65536, 1), (40000, 35947)])
def test_alignment_scratch_offsets_are_the_hand_written_formulas(exe, ns, nt):
    got = [int(v) for v in subprocess.run([exe, str(ns), str(nt)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == formula(ns, nt)
    assert all(o % 256 == 0 for o in got)


def test_an_array_of_no_elements_gets_nullptr(exe):
    assert subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split() == ["EMPTY", "1", "512"]

