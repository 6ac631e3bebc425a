#!/usr/bin/env python3
"""Record tests/golden/g11_render_digests.json: the SHA-256 of every output array of the three overlay entries on the small cases of
tests/render_cases.py (DIGEST_CASES), through the public Renderer API only - so this file and tests/render_cases.py, copied into a
checkout of an EARLIER commit, record what that commit draws.  That is how the file is made: from the commit before a change to
csrc/render.hip, never from the change itself; tests/test_render_digests.py then holds the change to those bytes.

One run records one device: the kernel emulator (--device cpu) or an MI355X (--device cuda:0).  The recording is merged into the
file: {"all": {...}} when the emulator's and the GPU's digests agree, else {"emu": {...}, "gfx950": {...}}.

usage:  python tools/make_golden_render.py [--device cpu|cuda:0] [--out tests/golden/g11_render_digests.json]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import render_cases as RC                                  # noqa: E402
from dynaboa_amd import _abi, _lib, assets                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda:0"])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g11_render_digests.json"))
    a = ap.parse_args()
    if a.device == "cpu":
        from emu.build_emu import build
        _lib.use_library(_abi.bind(ctypes.CDLL(build())))
    tabs = assets.make_synthetic_smpl(0)
    new = {name: RC.digests(case(a.device, tabs)) for name, case in RC.DIGEST_CASES.items()}
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        rec = {"emu": old["all"], "gfx950": old["all"]} if "all" in old else old
    rec["emu" if a.device == "cpu" else "gfx950"] = new
    if rec.get("emu") == rec.get("gfx950"):
        rec = {"all": new}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{a.out}: {sorted(rec)} ({sum(len(v) for v in new.values())} arrays on {a.device})")


if __name__ == "__main__":
    main()
