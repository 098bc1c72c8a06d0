"""Writes tests/golden/snapshot_image_digests.json: the SHA-256 and length of one exported image per snapshot kind
(tests/snapshot_digest_cases.py), from the emulator build of the engine.  The file pins the image formats: run this only on a
commit whose images are the reference -- before a change that must not move a byte, never after it.  The commit id written
into the file is the checkout's own HEAD, and a checkout with changes to csrc/ is refused:

    python tools/make_snapshot_digests.py [kind ...]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
sys.path[:0] = [ROOT, TESTS]
import hostsim  # noqa: E402
import snapshot_digest_cases as c  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main(kinds):
    git = lambda *a: subprocess.run(("git", "-C", ROOT) + a, check=True, capture_output=True, text=True).stdout.strip()
    if git("status", "--porcelain", "--", "summerset_amd/csrc"):
        sys.exit("summerset_amd/csrc differs from HEAD: the digests would not be that commit's")
    commit = git("rev-parse", "HEAD")
    O.build()
    hostsim.build()
    doc = c.golden() if os.path.exists(c.GOLDEN) else dict(images={})
    doc["commit"], doc["build"] = commit, "emulator (tests/hostsim)"
    for kind in kinds or c.KINDS:
        with hostsim.patched():
            img, shape = c.KINDS[kind]("cpu", O)
        doc["images"][kind] = dict(c.digest(img), shape=shape)
        print(kind, doc["images"][kind], flush=True)
    with open(c.GOLDEN, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
