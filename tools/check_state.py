"""Check a full-state checkpoint (HydraTrainer.save_state; multitask_hydranet_amd/checkpoint.py) without a GPU.

    python tools/check_state.py FILE

Reads and validates the file's structure, then verifies every tensor's checksum on the host (hn_state_checksum_host, a host function of
the library: no GPU call) and prints the manifest's summary.  Exit status 0: a good file; 1: unreadable / malformed, or a tensor's
words do not give the sums its manifest records (every such tensor is named)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
from multitask_hydranet_amd import checkpoint as C  # noqa: E402


def main(path: str) -> int:
    try:
        manifest, blob = C.read_file(path)
    except C.CheckpointError as e:
        print("check_state: %s" % e)
        return 1
    print("%s: %s" % (path, C.summary(manifest)))
    bad = C.verify_host(manifest, blob)
    for name in bad:
        print("check_state: CORRUPT %s: its words do not give the recorded checksum" % name)
    print("check_state: %s" % ("%i of %i tensors corrupt" % (len(bad), len(manifest["tensors"])) if bad else "every checksum verified"))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    sys.exit(main(ap.parse_args().file))
