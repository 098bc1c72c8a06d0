"""One exported EPaxos image from a fixed-seed `shadow` run (tests/ep_snapshot_cases.py: 130 groups, five replicas, window 8,
execution on) against the SHA-256 recorded in tests/golden/ep_snapshot_image_digests.json: the bytes of the image do not move,
and the device produces the emulator's.  The bodies of tests/test_ep_snapshot_digests.py (emulator, dev = "cpu") and
tests/test_zzzz_ep_snapshot_digests_gpu.py (device).  `python tests/ep_snapshot_digest_cases.py` writes the file from the
emulator: run it only on a commit whose image is the reference."""
import hashlib
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ep_snapshot_image_digests.json")
SHAPE = dict(G=130, R=5, W=8, K=3, T=20, seed=11)


def image(dev, oracle):
    """replica 0's image after the last tick of the run (the checks of `shadow` against the oracle run here too)"""
    import ep_snapshot_cases as c
    imgs = []
    c.shadow(dev, oracle, G=SHAPE["G"], R=SHAPE["R"], W=SHAPE["W"], K=SHAPE["K"], T=SHAPE["T"], seed=SHAPE["seed"], image_out=imgs)
    return imgs[-SHAPE["R"]]


def digest(img):
    return dict(sha256=hashlib.sha256(img).hexdigest(), bytes=len(img))


def check(dev, oracle):
    with open(GOLDEN) as f:
        want = json.load(f)["images"]["ep_replica"]
    got = digest(image(dev, oracle))
    assert got["bytes"] == want["bytes"] and got["sha256"] == want["sha256"], (got, want)


if __name__ == "__main__":
    import sys
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
    import hostsim
    from oracle import oracle as O
    O.build()
    hostsim.build()
    with hostsim.patched():
        d = digest(image("cpu", O))
    with open(GOLDEN, "w") as f:
        json.dump(dict(build="emulator (tests/hostsim)", images=dict(ep_replica=dict(d, shape=SHAPE))), f, indent=1, sort_keys=True)
        f.write("\n")
    print(d)
