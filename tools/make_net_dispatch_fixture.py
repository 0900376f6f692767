#!/usr/bin/env python3
"""Needs a GPU: the kernel label and issued-MFMA count of every net and batch size of tests/test_net_dispatch_gpu.py,
recorded from a given build of the engine library as the data fixture tests/golden/net_dispatch.json.

    python tools/make_net_dispatch_fixture.py [--lib path/to/libaz_engine.so] tests/golden/net_dispatch.json

--lib: record from another build (the fixture pins the dispatch of the build it was made from); default: the package's own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", help="the JSON file to write")
    ap.add_argument("--lib", default=None, help="an engine library build to record from")
    a = ap.parse_args()
    from alphazero_openspiel_amd import _lib, fusednet
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    import test_net_dispatch_gpu as T
    out = {"batches": list(T.BATCHES), "max_boards": T.MAX_BOARDS,
           "nets": {tag: {p: T.record(net, p) for p in fusednet.PRECISIONS} for tag, net in T.dispatch_nets().items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out, "from", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
