"""K19's LDS layout (csrc/fit_lds.hpp: k19_lds and the resident capacity) and its split of the groups into the two routes of the table
kernel (csrc/k19_split.hpp) on the CPU: a stand-alone program (tests/k19_layout_check.cpp, plain C++, no HIP) is compiled with the
address and undefined-behaviour sanitizers and run; what it prints is compared with sizes written out by hand below."""
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
BUDGET = 160 * 1024 - 256


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = tmp_path_factory.mktemp("k19") / "k19_layout_check"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'polars_ols_amd' / 'csrc'}", str(ROOT / "tests" / "k19_layout_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return [ln.split() for ln in out.splitlines()]


def _tri(n):
    return n * (n + 1) // 2


def _sizes(k, kc, rows):
    """tab, q, part, Gw, Gs, T, A, d0, rhs, Ri, Minv, bb, D, dz, dv, red, sc -- in doubles"""
    ne = _tri(kc + 1)
    return [rows * (k + 3), rows, max(ne, 256), _tri(k + 1) + k + 1, ne, kc, kc * (kc + 1), kc, kc, kc * kc, kc * kc, kc, k * (k + 1), k, k, 4, 4]


def test_lds_layout(lines):
    lds = {(int(ln[1]), int(ln[2]), int(ln[3])): [int(v) for v in ln[5:]] for ln in lines if ln[0] == "lds"}
    assert len(lds) == 2 * 61 + 1
    for (k, kc, rows), got in lds.items():
        assert got == list(itertools.accumulate([0] + _sizes(k, kc, rows))), (k, kc, rows)
    assert lds[(8, 9, 0)][:3] == [0, 0, 0] and lds[(8, 9, 15)][:3] == [0, 165, 180]
    # 15 categories at 8 features and an intercept: 6 184 bytes, two dozen workgroups to a CU's LDS
    assert 8 * lds[(8, 9, 15)][-1] == 8 * (180 + 256 + 54 + 55 + 9 + 90 + 9 + 9 + 81 + 81 + 9 + 72 + 8 + 8 + 4 + 4) == 7432
    assert 8 * lds[(31, 31, 0)][-1] < 48 * 1024


def test_resident_capacity(lines):
    cap = {(int(ln[1]), int(ln[2]), int(ln[3])): int(ln[5]) for ln in lines if ln[0] == "cap"}
    for (k, kc, budget), rows in cap.items():
        room = budget // 8 - sum(_sizes(k, kc, 0))
        assert rows == room // (k + 4) if room >= 0 else rows <= 0
    assert cap[(2, 3, BUDGET)] == (20448 - 335) // 6 == 3352 and cap[(2, 3, BUDGET)] < 12_000          # the 12 000-category group of the GPU test is global
    assert cap[(8, 9, BUDGET)] == 1641 and cap[(30, 31, 1024)] <= 0


def test_split_of_the_groups(lines):
    splits = [ln[1:] for ln in lines if ln[0] == "split"]
    # table rows 15, 200, 0, 12 000, 40 -> n_res, n_glb, max_res : the list of a mixed frame (resident groups first)
    assert splits[0] == ["5", "0", "12000", ":"]
    assert splits[1] == ["1", "4", "0", ":", "2", "0", "1", "3", "4"]
    assert splits[2] == ["4", "1", "200", ":", "0", "1", "2", "4", "3"]
    assert splits[3] == ["0", "5", "0", ":"]
    assert splits[4] == ["0", "0", "0", ":"]
