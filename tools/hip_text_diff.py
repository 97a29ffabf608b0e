#!/usr/bin/env python
"""Any box with the ROCm LLVM tools: is the device code of two builds the same? For every `*.hip.o` of two object directories
(build/obj/<hash of the flags>/ of two checkouts built with the same flags) the gfx950 code object is taken out of the object's
.hip_fatbin section, and the bytes of its .text are compared.

    python tools/hip_text_diff.py PARENT/build/obj/HASH THIS/build/obj/HASH

Prints one line per unit (`same <bytes>` or `DIFFERS <bytes> <bytes>`) and exits with status 1 when a unit other than those
named with --expect differs. What a commit that says "switches off: every other unit is untouched" runs
(profiles/site_pack/off_vs_parent.json)."""
import argparse, os, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")


def text_of(obj: str, tmp: str) -> bytes:
    fat, co, text = (os.path.join(tmp, n) for n in ("fat.bin", "code.co", "text.bin"))
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.devnull], check=True)
    listed = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--list", "--type=o", "--input=" + fat], check=True, capture_output=True, text=True)
    target = [t for t in listed.stdout.split() if "gfx950" in t][0]
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + target, "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text", co, text], check=True)
    return open(text, "rb").read()


ap = argparse.ArgumentParser()
ap.add_argument("parent")
ap.add_argument("this")
ap.add_argument("--expect", default="", help="comma list of units that may differ, e.g. site_summary.hip.o")
args = ap.parse_args()
allowed = set(args.expect.split(","))
bad = 0
with tempfile.TemporaryDirectory() as tmp:
    for name in sorted(f for f in os.listdir(args.parent) if f.endswith(".hip.o")):
        a, b = text_of(os.path.join(args.parent, name), tmp), text_of(os.path.join(args.this, name), tmp)
        if a == b:
            print(name, "same", len(a))
        else:
            print(name, "DIFFERS", len(a), len(b))
            bad += name not in allowed
sys.exit(1 if bad else 0)
