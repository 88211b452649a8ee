"""Generates tests/golden/step_sequence_parent.json: the launch sequence of one training step as
the parent commit's library issued it, before csrc/net.cpp was split, for every case of
tests/step_sequence_cases.py.

    python tests/golden/make_step_sequence_fixture.py <libseg_hip.so built from the parent commit>

Needs the GPU: the library is loaded through SEG_HIP_LIB in a child process, which runs each case
with the profiler on and reads seg_profile_dump and seg_counter. The fixture holds the recorded
rows only; tests/test_gpu_step_sequence.py runs the same cases on the working tree's library."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(REPO, "iv2019-boosting-semantic-segmentation-with-weak-labels_amd")
OUT = os.path.join(HERE, "step_sequence_parent.json")


def child():
    sys.path[:0] = [REPO, PKG, os.path.join(REPO, "tests")]
    import step_sequence_cases as cases
    out = {}
    for name in cases.CASE_NAMES:
        rows, counters, _ = cases.record(name)
        out[name] = {"counters": counters, "rows": rows}
        print(name, len(rows), "records", counters, file=sys.stderr)
    # the switches of cases 1 to 3 really switched: the pin cannot go vacuous
    a, b, c = (out[n]["counters"] for n in cases.CASE_NAMES[:3])
    assert a["lbf_layers"] > 0 and b["lbf_layers"] == 0 and c["lbf_layers"] == 0, (a, b, c)
    assert b["premask_launches"] > 0 and c["premask_launches"] == 0, (b, c)
    assert a["premask_launches"] > 0, a
    assert out[cases.CASE_NAMES[0]]["rows"] != out[cases.CASE_NAMES[1]]["rows"]
    assert out[cases.CASE_NAMES[1]]["rows"] != out[cases.CASE_NAMES[2]]["rows"]
    with open(OUT, "w") as f:   # one line per case
        f.write('{"columns":["class","conv","work","bytes"],"cases":{\n')
        f.write(",\n".join(json.dumps(n) + ":" + json.dumps(out[n], separators=(",", ":"))
                           for n in cases.CASE_NAMES))
        f.write("\n}}\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        child()
    else:
        env = dict(os.environ, SEG_HIP_LIB=os.path.abspath(sys.argv[1]))
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env).returncode)
