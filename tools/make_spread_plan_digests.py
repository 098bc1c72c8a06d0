"""Writes tests/golden/spread_plan_digests.json: per case, rank and exchange of layout L2 the split sizes and the SHA-256 of the
messages' send and receive offsets (tests/spread_plan_cases.py), from the Python plan builders over the emulator build of the
engine.  The file pins the plans: run this only on a commit whose plans are the reference -- before a change that must not move
an offset, never after it.  The commit id written into the file is the checkout's own HEAD, and a checkout with changes to
summerset_amd/ is refused:

    python tools/make_spread_plan_digests.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
sys.path[:0] = [ROOT, TESTS]
import hostsim  # noqa: E402
import spread_plan_cases as c  # noqa: E402


def main():
    git = lambda *a: subprocess.run(("git", "-C", ROOT) + a, check=True, capture_output=True, text=True).stdout.strip()
    if git("status", "--porcelain", "--", "summerset_amd"):
        sys.exit("summerset_amd differs from HEAD: the digests would not be that commit's")
    commit = git("rev-parse", "HEAD")
    hostsim.build()
    lines = []
    for name, (make, case) in c.CASES.items():
        with hostsim.patched():
            ranks = make(case)
            try:
                rec = c.record(ranks)
            finally:
                c.close(ranks)
        lines.append("  %s: %s" % (json.dumps(name), json.dumps(rec, sort_keys=True, separators=(",", ":"))))
        print(name, len(lines[-1]), "bytes", flush=True)
    with open(c.GOLDEN, "w") as f:                                 # one case per line
        f.write('{\n "build": "emulator (tests/hostsim)",\n "commit": %s,\n "cases": {\n%s\n }\n}\n' % (json.dumps(commit), ",\n".join(lines)))
    assert c.golden()["commit"] == commit


if __name__ == "__main__":
    main()
