"""The scratch carver (csrc/scratch_carve.hpp), the layouts of the two cached tables (csrc/table_layout.hpp: the build view and the view a
cache hit takes must agree), K17's resident / global split of the groups (csrc/k17_split.hpp) and the LDS layouts of the one-wave solve
kernels (csrc/fit_lds.hpp: the kernel's offsets and the launcher's total come from one function) on the CPU: a
stand-alone program (tests/carve_check.cpp, plain C++, no HIP) is compiled with the address and undefined-behaviour sanitizers and run;
what it prints is compared with offsets and totals written out by hand below.  The program writes every region it carved end to end
into a buffer of exactly the total, so a region that reaches past the allocation is a sanitizer report and a failed run."""
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def r(b):
    """a region's room: its bytes rounded up to 256"""
    return (b + 255) // 256 * 256


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = tmp_path_factory.mktemp("carve") / "carve_check"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'polars_ols_amd' / 'csrc'}", str(ROOT / "tests" / "carve_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return [ln.split() for ln in out.splitlines()]


@pytest.fixture(scope="module")
def printed(lines):
    named = {ln[0]: [int(v) for v in ln[1:]] for ln in lines if ln[0] not in ("split", "lds")}
    return named, [ln[1:] for ln in lines if ln[0] == "split"]


@pytest.fixture(scope="module")
def lds(lines):
    """the LDS layouts of the one-wave solve kernels (csrc/fit_lds.hpp): name -> the offsets of the areas in order, then the total (doubles)"""
    return {ln[1]: [int(v) for v in ln[3:]] for ln in lines if ln[0] == "lds"}


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


def test_a_kept_region_keeps_its_room_when_it_is_not_wanted(printed):
    named, _ = printed
    # the staged outputs of a host batch as api.hip laid them out before the carver: q += coefb; q += colb; q += colb; total
    # coefb + 2 * colb + statb whatever is wanted (5 groups, 7 columns, 415 rows, f32)
    coefb, colb, statb = r(4 * 5 * 7), r(4 * 415), r(4 * 5)
    total = coefb + 2 * colb + statb
    assert named["kept_all"] == [0, coefb, coefb + colb, coefb + 2 * colb, total]
    assert named["kept_mid"] == [0, -1, coefb + colb, coefb + 2 * colb, total]          # pred unwanted: resid and status do not move
    assert named["kept_end"] == [0, coefb, -1, -1, total]                               # unwanted at the end: the total stays
    assert named["kept_none"] == [-1, -1, -1, -1, total]


def test_a_gap_is_room_without_a_slot(printed):
    named, _ = printed
    assert named["gap"] == [256, 256 + r(8 * 33) + 256]


def test_a_run_of_columns_is_one_region(printed):
    named, _ = printed
    colb = r(4 * 415)                                                                   # cols + colb * j
    assert named["columns"] == [0, 3 * colb, 4 * colb, 2 * colb, 5 * colb, 5 * colb]    # ... and a wanted region of 0 bytes has an address


def test_chunk_tables_as_built_and_as_found_again(printed):
    named, _ = printed
    # api_dynamic.hip before the carver, 5 groups (40-byte records), 37 chunks (24-byte records), 9 000 rows:
    # b_groups + b_chunks + b_order + 2 * b_cnt + b_sc + b_sb + b_co + 256; a hit read groups at 0, chunks at b_groups, order behind them
    b_groups, b_chunks, b_order, b_cnt = r(40 * 5), r(24 * 37), r(4 * 37), r(4 * 9000)
    slabs = (9000 + 255) // 256
    b_sc, b_sb, b_co = r(4 * slabs), r(8 * (slabs + 1)), r(8 * (5 + 1))
    head = [0, b_groups, b_groups + b_chunks]
    t_cnt = b_groups + b_chunks + b_order
    plain = head + [-1] * 5 + [t_cnt + 256]
    host = head + [t_cnt, t_cnt + b_cnt, -1, -1, -1, t_cnt + 2 * b_cnt + 256]
    scr = t_cnt + 2 * b_cnt
    dev = head + [t_cnt, t_cnt + b_cnt, scr, scr + b_sc, scr + b_sc + b_sb, scr + b_sc + b_sb + b_co + 256]
    assert named["chunks_plain"] == plain + plain
    assert named["chunks_host_valid"] == host + host
    assert named["chunks_device_valid"] == dev + dev


def test_segment_tables_as_built_and_as_found_again(printed):
    named, _ = printed
    # api.hip before the carver, 40 segments with 136 bytes of partial results each: the whole frame (4 groups) keeps n_seg + 1 offsets,
    # a size-class list (3 groups) a (start, end) pair per segment; map, first, then the extra area
    for name, b_so, items in (("seg_frame", r(8 * 41), 4), ("seg_classes", r(8 * 80), 3)):
        b_sm, b_sf = r(4 * 40), r(4 * (items + 1))
        view = [0, b_so, b_so + b_sm, b_so + b_sm + b_sf, b_so + b_sm + b_sf + r(136 * 40)]
        assert named[name] == view + view


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


def _tri(n):
    return n * (n + 1) // 2


def _laid_out(got, sizes):
    """the areas follow each other in the struct's order, none empty, none over the next: offsets = running sums of the sizes the kernel
    uses, and the total ends the last one"""
    assert all(s > 0 for s in sizes)
    assert got == list(itertools.accumulate([0] + sizes)), (got, sizes)
    assert all(a < b for a, b in zip(got, got[1:]))


def test_lds_layouts_of_the_absorb_solves(lds):
    for k in range(1, 32):
        # Gs, T_jj (K16: then n), A, d0, rhs, Ri
        _laid_out(lds[f"k16_{k}"], [_tri(k + 1), k + 1, k * (k + 1), k, k, k * k])
        _laid_out(lds[f"k17_{k}"], [_tri(k + 1), k, k * (k + 1), k, k, k * k])
        # the launchers' own sums before there was a layout function (k16_solve_lds; k17_solve_launch)
        assert lds[f"k16_{k}"][-1] == (k + 1) * (k + 2) // 2 + k + 1 + k * (k + 1) + 2 * k + k * k
        assert lds[f"k17_{k}"][-1] == (k + 1) * (k + 2) // 2 + k + k * (k + 1) + 2 * k + k * k


def test_lds_layout_of_the_glsar_solve(lds):
    for kt in range(1, 32):
        T = kt + 1
        ne = _tri(T)
        # Ss, Cs, z1, zn, Gm, A, rhs, d0, b0, vv, tn, td, Ri, ij (two int32 per double)
        _laid_out(lds[f"k18_{kt}"], [ne, T * T, T, T, ne, kt * (kt + 1), kt, kt, kt, T, T, T, kt * kt, (ne + 1) // 2])
        assert lds[f"k18_{kt}"][1] == ne                                             # C right behind S: the kernel sums both as one run
        assert lds[f"k18_{kt}"][-1] == 2 * ne + T * T + 5 * T + kt * (kt + 1) + 3 * kt + kt * kt + (ne + 1) // 2


def test_lds_layout_of_the_iv_solve(lds):
    triples = [(kx, kx, kx + 1) for kx in range(1, 31)] + [(6, 8, 10), (2, 29, 30), (30, 31, 31), (15, 16, 31)]
    for kx, L, T in triples:
        # Gs (+ n), A, d0, B, Gm2, A2, rhs2, d02, Ri, tmp
        got = lds[f"k14_{kx}_{L}_{T}"]
        _laid_out(got, [_tri(T + 1) + 1, L * (L + 1), L, L * (kx + 1), _tri(kx + 1), kx * (kx + 1), kx, kx, kx * kx, L])
        assert got[-1] == _tri(T + 1) + 1 + L * (L + 1) + 2 * L + L * (kx + 1) + _tri(kx + 1) + kx * (kx + 1) + 2 * kx + kx * kx
    assert 8 * lds["k14_6_8_10"][-1] == 2632 and 8 * lds["k14_30_31_31"][-1] == 39440     # the figures in k14_iv.hip's header
