#!/usr/bin/env python3
"""One sha256 per csrc/*.hip over its gfx950 device assembly, to show that a host-side change leaves every kernel as it was: run it
on two revisions and compare the outputs line for line.  Needs hipcc, no GPU.  (Object files carry a build id: the assembly text is
what compares.)

usage: python tools/device_code_digest.py [--jobs N] [--keep DIR] [--per-kernel] [file.hip ...]

Each file is compiled from inside csrc/ with the flags of build() and --offload-device-only -S; the digest is over that text with the
__hip_cuid_<hash> symbol's hash removed (it depends on where the checkout and the output lie).  --keep DIR leaves the .s files in
DIR (to diff two revisions where a digest moved).

--per-kernel prints, per file, one line per kernel instead: sha256, instruction lines, symbol.  That shows identity across a change that
renames kernels or moves them within a file: compare the sorted (sha256, instruction lines) columns of two revisions.  The hash is over
the kernel's function body and its .amdhsa_kernel block, comments stripped, with the kernel's own mangled name and the numbers of the
.LBB<n>_ / .Lfunc_*<n> labels (the function's position in the file) replaced by fixed tokens."""
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


def kernels(text):
    """(sha256, instruction lines, symbol) of every kernel in the assembly text, in file order"""
    lines = text.decode().split("\n")
    rows = []
    for end, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        sym = m.group(1)
        start = max(i for i in range(end) if lines[i].startswith(sym + ":"))
        stop = next(i for i in range(end, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        body = [l.split(";")[0].rstrip() for l in lines[start:stop + 1]]
        body = [re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", re.sub(r"\.LBB\d+_", ".LBB_", l.replace(sym, "KERNEL"))) for l in body if l]
        count = sum(1 for l in body if l[0] in " \t" and not l.lstrip().startswith("."))       # neither a label nor a directive
        rows.append((hashlib.sha256("\n".join(body).encode()).hexdigest(), count, sym))
    return rows


def assemble(hipcc, name, outdir, per_kernel=False):
    out = os.path.join(outdir, name[:-len(".hip")] + ".s")
    subprocess.check_call([hipcc] + FLAGS + [name, "-o", out], cwd=CSRC)
    with open(out, "rb") as f:
        text = f.read()
    if per_kernel:
        return kernels(text)
    # the compilation unit id hashes the paths and options of the command, not the code: leave it out
    return hashlib.sha256(re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_", text)).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", metavar="DIR")
    ap.add_argument("--per-kernel", action="store_true")
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
            digests = list(pool.map(lambda n: assemble(hipcc, n, outdir, args.per_kernel), names))
    if args.per_kernel:
        for n, rows in zip(names, digests):
            print(f"# {n}: {len(rows)} kernels")
            for d, count, sym in rows:
                print(f"{d}  {count}  {sym}")
        return 0
    total = hashlib.sha256()
    for n, d in zip(names, digests):
        total.update(d.encode())
        print(f"{d}  {n}")
    print(f"{total.hexdigest()}  all of the above")


if __name__ == "__main__":
    sys.exit(main())
