"""CPU: the pairs of tests/test_twoview_motion_gpu.py, through RecoverPoseTwoView over the CPU oracle behind the C-ABI
(tests/cpp/oracle_abi.cpp; tests/cpp/twoview_motion_driver.cpp built without its batch half, which that file has no entry point
for), reach what the GPU comparison needs: both branches of RecoverPoseTwoView, a pair without an essential matrix, a homography
branch that accepts a solution and one that does not."""
import os
import subprocess

import oracle
import twoview_motion_cases as MC


def test_the_pairs_reach_both_branches(tmp_path):
    so = oracle.build()
    exe = MC.build_driver(str(tmp_path / "twoview_motion_driver"), [os.path.join(MC.CPP, "oracle_abi.cpp"), so, "-Wl,-rpath," + os.path.dirname(so)],
                          defines=["EACHAM_MOTION_SINGLE_ONLY"])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    MC.write_input(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    single, pose = MC.read_groups(fout, [MC.SINGLE, MC.POSE])
    MC.assert_coverage(single, pose)
