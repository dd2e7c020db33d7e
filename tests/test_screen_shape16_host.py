"""CPU: the lane map of the screen sweep's 16x16x128 chains (eacham_amd/csrc/match_screen.hpp: frag16_src, query16_src, the two plane
offsets, acc16_row), compiled on its own with g++ and EXECUTED by tests/cpp/screen_shape16_driver.cpp on stored tiles built the way
the upload kernel builds them. Three images carry the 13-bit identifier 256 row + k of every position in their 6-bit codes, so what
a lane reads says where it came from; random tiles carry a 64 x 32 x 256 product."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shape16") / "screen_shape16_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "screen_shape16_driver.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-400:], r.stderr[-400:])
    return json.loads(r.stdout)


def test_a_lane_reads_one_k_block_of_its_row(report):
    """For every (u, S, lane) the 32 codes read are those of row 16 u + (lane & 15), one K block of step S, ascending, inside the tile."""
    assert report["fragments"] == 256
    assert (report["bad_bounds"], report["bad_row"], report["bad_block"], report["bad_step"]) == (0, 0, 0, 0), report


def test_the_fragments_cover_the_tile_once(report):
    """The 2 x 2 x 64 lane-fragments name every (row, K block) of the tile exactly once."""
    assert report["bad_cover"] == 0, report


def test_the_query_side_names_the_same_k_block(report):
    assert report["bad_query"] == 0, report


def test_a_lane_holds_one_group_of_four_rows(report):
    """Lane (j, kg)'s four accumulators of row half u are the stored rows of group 4 u + kg, in order."""
    assert report["bad_group"] == 0, report


def test_the_product_in_this_order_is_the_integer_distance(report):
    """64 query rows x 32 train rows x 256 codes accumulated chain by chain as the kernel does (C-init |M_b|^2 / 2, two K = 128 steps,
    the query's sign flipped) = |M_a - M_b|^2 of screen::decode, on random codes and with dimensions 129 .. 255 padded with code 0."""
    assert report["products"] == 3 * 64 * 32 and report["bad_product"] == 0, report
