"""GPU: the batch adapters of the second half of RecoverPoseTwoView — RecoverPoseBatch and TwoViewMotionBatch
(include/eacham/TwoViewHip.hpp, one eacham_two_view_batch call for the whole list) and
ReconstructionManagerHip::RecoverPoseTwoViewBatch (include/eacham/ReconstructionHip.hpp: three device calls for the whole list) —
against RecoverPose / RecoverPoseTwoView pair by pair, on the stand-ins of tests/cpp/ref_standins.hpp, in both directions of 8
seeded pairs (tests/twoview_motion_cases.py: planar, general and partly planar ones, one with fewer than 5 matches, the sizes 57,
130, 300 and 301): every field identical, byte for byte — transform, R, t, good, mask, the matches with their points."""
import os
import subprocess

import pytest

import twoview_motion_cases as MC


@pytest.mark.gpu
def test_batch_adapters_equal_the_single_pair_ones(tmp_path):
    lib = os.path.join(MC.ROOT, "eacham_amd", "lib")
    exe = MC.build_driver(str(tmp_path / "twoview_motion_driver"), ["-L" + lib, "-leacham_hip", "-Wl,-rpath," + lib])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    MC.write_input(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    single, pose1, batch, motion, poseB = MC.read_groups(fout, [MC.SINGLE, MC.POSE, MC.SINGLE, MC.SINGLE, MC.POSE])
    MC.assert_coverage(single, pose1)                     # both branches are exercised (checked on the CPU first: test_twoview_motion_reference.py)
    sizes = [n for n, _, _ in MC.PAIRS for _ in range(2)]
    for what, got, want, fields in (("RecoverPoseTwoViewBatch", batch, single, MC.SINGLE), ("TwoViewMotionBatch", motion, single, MC.SINGLE),
                                    ("RecoverPoseBatch", poseB, pose1, MC.POSE)):
        for d, (g, w) in enumerate(zip(got, want)):
            for name in fields:
                assert g[name] == w[name], f"{what}, directed pair {d} ({sizes[d]} matches): {name} differs"
