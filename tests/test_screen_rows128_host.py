"""CPU: the query-side map of the screen sweep with 128 rows per wave (eacham_amd/csrc/match_screen.hpp: query16_tile, query16_src,
query16_block, query16_wave_row over eight sub-tiles), compiled on its own with g++ and EXECUTED by
tests/cpp/screen_rows128_driver.cpp on stored tiles built the way the upload kernel builds them. Three images of the wave's four
stored query tiles carry the 15-bit identifier 256 row + k of every position in their 6-bit codes, so what a lane reads says where it
came from; random tiles carry a 128 x 32 x 256 product in the kernel's order, with its one set of accumulators and its tail per
wave-block."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows128") / "screen_rows128_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "screen_rows128_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    return json.loads(r.stdout)


def test_a_lane_reads_its_row_of_the_wave_and_the_train_sides_k_block(report):
    """For every (s8, S, lane) the 32 codes read are those of the wave's row 16 s8 + (lane & 15), the K block that the train side gives
    the lane in step S, ascending, inside stored tile s8 >> 1 of the wave's four."""
    assert report["fragments"] == 8 * 2 * 64
    assert (report["bad_bounds"], report["bad_row"], report["bad_block"]) == (0, 0, 0), report


def test_the_fragments_cover_the_waves_rows_once(report):
    """The 8 x 2 x 64 lane-fragments name every (row, K block) of the 128 rows exactly once."""
    assert report["bad_cover"] == 0, report


def test_a_sub_tile_lies_in_one_wave_block(report):
    """Sub-tile s8 is sub-tile s8 & 3 of wave-block s8 >> 2: its rows lie in that block of 64 and its stored tile is one of the block's two."""
    assert report["bad_wave_block"] == 0, report


def test_the_tail_gives_every_lane_the_row_of_its_number(report):
    """In the tail of wave-block H, lane t keeps the minima of sub-tile 4 H + (t >> 4) and owns row 64 H + t: that sub-tile's column t & 15."""
    assert report["bad_owner"] == 0, report


def test_the_product_in_this_order_is_the_integer_distance(report):
    """128 query rows x 32 train rows x 256 codes through ONE set of accumulators in the order (0,0) (1,0) (0,1) (1,1), row half 0 read
    behind step 2 and row half 1 behind step 3, = |M_a - M_b|^2 of screen::decode, on random codes and with dimensions 129 .. 255 padded
    with code 0; the tail's join over a row's column gives the row's minimum over the tile."""
    assert report["products"] == 2 * 128 * 32 and report["bad_product"] == 0, report
    assert report["minima"] == 2 * 128 and report["bad_minimum"] == 0, report
