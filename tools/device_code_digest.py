#!/usr/bin/env python3
"""One sha256 per csrc/*.hip over its gfx950 device assembly, to show that a host-side change leaves every kernel as it was: run it
on two revisions and compare the outputs line for line.  Needs hipcc, no GPU.  (Object files carry a build id: the assembly text is
what compares.)

usage: python tools/device_code_digest.py [--jobs N] [--keep DIR] [file.hip ...]

Each file is compiled from inside csrc/ with the flags of build() and --offload-device-only -S; the digest is over that text with the
__hip_cuid_<hash> symbol's hash removed (it depends on where the checkout and the output lie).  --keep DIR leaves the .s files in
DIR (to diff two revisions where a digest moved)."""
import argparse
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-subtitle-extractor_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-device-only", "-S"]


def assemble(hipcc, name, outdir):
    out = os.path.join(outdir, name[:-len(".hip")] + ".s")
    subprocess.check_call([hipcc] + FLAGS + [name, "-o", out], cwd=CSRC)
    with open(out, "rb") as f:
        text = f.read()
    # the compilation unit id hashes the paths and options of the command, not the code: leave it out
    return hashlib.sha256(re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_", text)).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", metavar="DIR")
    ap.add_argument("files", nargs="*")
    args = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    names = sorted(os.path.basename(f) for f in args.files) or sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp:
        outdir = tmp
        if args.keep:
            outdir = os.path.abspath(args.keep)
            os.makedirs(outdir, exist_ok=True)
        with concurrent.futures.ThreadPoolExecutor(max(1, args.jobs)) as pool:
            digests = list(pool.map(lambda n: assemble(hipcc, n, outdir), names))
    total = hashlib.sha256()
    for n, d in zip(names, digests):
        total.update(d.encode())
        print(f"{d}  {n}")
    print(f"{total.hexdigest()}  all of the above")


if __name__ == "__main__":
    sys.exit(main())
