"""The host plan of a fixed-base sum without a GPU (csrc/fb_sum_plan.hpp: the grids, the fold of the bucket sums, the buffer sizes and the
layout of the tail that fb_msm_launch carves and FbSumBufs::reserve sizes) in a stand-alone program - built plain and under the address
and undefined-behaviour sanitizers - against the formulas as the callers and the launcher each spelled them before the plan existed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS = [1, 2, 767, 768, 769, 4095, 4096, 4097, 12288, 12289, 1 << 18, 1 << 20, (1 << 21) + 3, 1 << 24, 1 << 26]
SLICES = [1024, 12288]
FOLD_PER_MIN = [2, 11, 64]
# the constants of msm_fixed.hpp, msm.hpp and the 12 x 32-bit field form, as they stood
PARTS, TERMS_PER_BLOCK, WINDOWS, FOLD_MAX_GROUPS, SAVE2_WORDS, JAC_BYTES = 128, 1024, 16, 128, 48, 144


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fbs") / ("fb_sum_plan_main_" + request.param))
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g"] + san + ["-I", os.path.join(ROOT, "kzg_rs_amd", "csrc"), "-o", exe,
                                                                       os.path.join(ROOT, "tests", "host", "fb_sum_plan_main.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        return [int(x) for x in out.stdout.split()]
    return run


def test_constants_are_the_kernels(plan):
    assert plan("constants") == [PARTS, 12288, TERMS_PER_BLOCK, 11, 4 * PARTS + 2, FOLD_MAX_GROUPS, SAVE2_WORDS, JAC_BYTES, WINDOWS]


def fb_max_blocks(n_entries, L):
    return PARTS + (n_entries + L - 1) // L


def msm_large_tail_groups(Z, per):
    groups = (Z + per - 1) // per
    gp = 2
    while gp < groups:
        gp <<= 1
    return groups, gp


def fb_tail_bytes(gp):
    return 4 * (FOLD_MAX_GROUPS + 256 * gp * SAVE2_WORDS + 2 * 256 * SAVE2_WORDS) + 2 * JAC_BYTES + 256


@pytest.mark.parametrize("L", SLICES)
@pytest.mark.parametrize("fold_per_min", FOLD_PER_MIN)
def test_every_field_is_what_callers_and_launcher_derived(plan, L, fold_per_min):
    for n in TERMS:
        nb, Z, per, groups, gp, entries, save_words, tail_bytes, off_flags, off_part, off_buckets, off_wsums, save_fits, touched = plan("plan", n, L, fold_per_min)
        at = (n, L, fold_per_min)
        # the launcher and its five callers
        assert nb == (n + TERMS_PER_BLOCK - 1) // TERMS_PER_BLOCK, at
        assert entries == WINDOWS * n, at
        assert Z == fb_max_blocks(WINDOWS * n, L), at
        assert per == max(fold_per_min, (Z + FOLD_MAX_GROUPS - 1) // FOLD_MAX_GROUPS), at
        assert (groups, gp) == msm_large_tail_groups(Z, per), at
        assert save_words == Z * 256 * SAVE2_WORDS, at
        assert tail_bytes == fb_tail_bytes(gp), at
        # the launcher's pointers: flags = tmp | part = flags + MSM_FOLD_MAX_GROUPS words | buckets = part + 256 gp records |
        # wsums = 64 bytes behind the [2][256] bucket records
        assert off_flags == 0 and off_part == 4 * FOLD_MAX_GROUPS, at
        assert off_buckets == off_part + 4 * 256 * gp * SAVE2_WORDS, at
        assert off_wsums == off_buckets + 4 * 2 * 256 * SAVE2_WORDS + 64, at
        # what the fold's kernels require
        assert groups <= 128, at
        assert gp & (gp - 1) == 0 and max(2, groups) <= gp <= 128, at
        # four regions, in this order, disjoint, aligned, inside the tail
        regions = [(off_flags, 4 * gp), (off_part, 4 * 256 * gp * SAVE2_WORDS), (off_buckets, 4 * 2 * 256 * SAVE2_WORDS), (off_wsums, 2 * JAC_BYTES)]
        end = 0
        for off, size in regions:
            assert off % 16 == 0 and off >= end, at
            end = off + size
        assert end <= tail_bytes, at
        assert touched == sum(size for _, size in regions), at      # (the program returns 3 if a byte has two owners)
        # kzg_g1_msm_setup takes the fixed form while the save area stays within 2 GiB
        assert save_fits == int(fb_max_blocks(WINDOWS * n, L) * 256 * SAVE2_WORDS * 4 <= 2 << 30), at
        assert save_fits == int(save_words * 4 <= 2 << 30), at


def test_the_default_plan_is_the_product_builds(plan):
    """fb_sum_plan(terms) as the prover and the prepared-set callers take it: 12 288-entry slices, eleven layers per fold thread; and the
    sizes at which the 2 GiB bound switches kzg_g1_msm_setup to the window form lie where they lay"""
    assert plan("plan", 4096, 12288, 11)[:5] == [4, 134, 11, 13, 16]
    assert plan("plan", 1 << 24, 12288, 11)[12] == 1 and plan("plan", 1 << 26, 12288, 11)[12] == 0
    assert plan("plan", 1 << 21, 1024, 11)[12] == 1 and plan("plan", 1 << 24, 1024, 11)[12] == 0
