"""Records the sample streams of tests/graph_verify_cases.py as include/eacham/TwoViewHip.hpp draws them on the host:

    python tests/golden/make_graph_verify_golden.py [include dir of the commit to record from]

graph_verify_streams.json was recorded from the commit BEFORE the streams became shared host/device functions
(include/eacham/CvSampling.hpp): tests/test_graph_verify_reference.py holds the shared functions to it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import graph_verify_cases as GC  # noqa: E402


def record(exe=None):
    out = {}
    for name, g, its in (("small", GC.small(), {"homography": 72, "essential": 89}), ("large", GC.large(), {"homography": 3, "essential": 3})):
        pts = GC.gather(g)
        for kind, m in GC.M.items():
            for sampling in ("opencv", "counter"):
                s = GC.host_samples(pts, m, kind == "homography", sampling, its[kind], g["seeds"], exe)
                out[f"{name}/{kind}/{sampling}/{its[kind]}"] = [x.tolist() for x in s]
    for n, m, its in ((4, 4, 72), (8, 4, 72), (5, 5, 89)):   # getSubset without a checkSubset
        z = [(GC.np.zeros((n, 2)), GC.np.zeros((n, 2)))]
        out[f"unchecked/{n}/{m}/{its}"] = GC.host_samples(z, m, False, "opencv", its, [0], exe)[0].tolist()
    return out


if __name__ == "__main__":
    exe = GC.samples_exe(sys.argv[1]) if len(sys.argv) > 1 else None
    with open(os.path.join(HERE, "graph_verify_streams.json"), "w") as f:
        json.dump(record(exe), f, separators=(",", ":"))
        f.write("\n")
