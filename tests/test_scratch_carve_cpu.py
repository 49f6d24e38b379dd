"""The scratch carver (csrc/scratch_carve.hpp) and K17's resident / global split of the groups (csrc/k17_split.hpp) on the CPU: a
stand-alone program (tests/carve_check.cpp, plain C++, no HIP) is compiled with the address and undefined-behaviour sanitizers and run;
what it prints is compared with offsets and totals written out by hand below.  The program writes every region it carved end to end
into a buffer of exactly the total, so a region that reaches past the allocation is a sanitizer report and a failed run."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def r(b):
    """a region's room: its bytes rounded up to 256"""
    return (b + 255) // 256 * 256


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = tmp_path_factory.mktemp("carve") / "carve_check"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'polars_ols_amd' / 'csrc'}", str(ROOT / "tests" / "carve_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    lines = [ln.split() for ln in out.splitlines()]
    named = {ln[0]: [int(v) for v in ln[1:]] for ln in lines if ln[0] != "split"}
    return named, [ln[1:] for ln in lines if ln[0] == "split"]


def test_offsets_and_totals(printed):
    named, _ = printed
    # counts, parts, reduced matrices: 37 segments of 5 groups, 45 doubles each
    assert named["enet_split"] == [0, r(8 * 37), r(8 * 37) + r(8 * 37 * 45), r(8 * 37) + r(8 * 37 * 45) + r(8 * 5 * 45)]
    # two sizes, each used twice in sequence
    b1, b2 = 8 * 5 * 33 + 8, 8 * 5 * 12 + 8
    assert named["twice"] == [0, r(b1), r(b1) + r(b2), 2 * r(b1) + r(b2), 2 * (r(b1) + r(b2))]
    # a raw region of 100 doubles + 100 int32, an exact multiple of 256 (no padding behind it), one byte
    assert named["raw"] == [0, r(1200), r(1200) + 512, r(1200) + 512 + 256]


def test_a_zero_size_region_takes_no_room(printed):
    named, _ = printed
    n = r(4 * 1001 + 4)
    assert named["absent"] == [0, -1, n, 2 * n]                   # its slot is nullptr, the next region starts where it would have


def test_an_absent_region_aliases_its_stand_in(printed):
    named, _ = printed
    # nothing is split: the reduced matrices ARE the parts, and the buffer ends behind the parts
    assert named["enet_whole"] == [0, r(8 * 5), r(8 * 5), r(8 * 5) + r(8 * 5 * 45)]
    assert named["enet_split"][2] != named["enet_split"][1]


def test_a_repeat_lays_the_same_tables_out_once_per_column(printed):
    named, _ = printed
    one = r(4 * 7) + r(8 * 8) + r(4 * 415 + 4)                    # counts, firsts, row index
    assert named["repeat"] == [0, r(4 * 7), r(4 * 7) + r(8 * 8), one, one + r(4 * 7), one + r(4 * 7) + r(8 * 8), 2 * one]


def test_every_offset_is_a_multiple_of_256(printed):
    named, _ = printed
    for name, values in named.items():
        assert all(v == -1 or v % 256 == 0 for v in values), (name, values)


def test_k17_split_of_the_groups(printed):
    _, splits = printed
    # groups of 60, 200, 0, 7600 and 120 rows -> n_res, max_res, max_glb : the list of a mixed frame (resident groups first)
    assert splits[0] == ["5", "7600", "0", ":"]                                   # cap 10 000: all resident, no list
    assert splits[1] == ["0", "0", "7600", ":"]                                   # 60, 200, 7600 rows under cap 10: none
    assert splits[2] == ["4", "200", "7600", ":", "0", "1", "2", "4", "3"]        # cap 200: the empty group counts as resident
    assert splits[3] == ["0", "0", "7600", ":"]                                   # cap -1: not even the empty group
