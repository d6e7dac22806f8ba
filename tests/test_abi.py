"""The C-ABI library builds for gfx950 (cross-compile, no GPU), loads, and exports every symbol declared in
include/vse_hip.h; record layouts agree between ir.py and the C structs.  CPU only — no compute calls."""
import ctypes
import glob
import os
import re

from vse_amd import engine, ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "vse_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vse_[a-z_]+)\s*\(", src)))


def product_env_reads():
    """Every VSE_* environment variable the product reads: getenv("VSE_...") in csrc/, os.environ / os.getenv in the package's modules."""
    pkg = os.path.join(ROOT, "video-subtitle-extractor_amd")
    names = set()
    for f in glob.glob(os.path.join(pkg, "csrc", "*.h*")):          # .hip and .h
        names |= set(re.findall(r'getenv\(\s*"(VSE_[A-Z0-9_]+)"', open(f).read()))
    for f in glob.glob(os.path.join(pkg, "*.py")):
        src = open(f).read()
        names |= set(re.findall(r'os\.(?:environ(?:\.get)?|getenv)\s*[(\[]\s*["\'](VSE_[A-Z0-9_]+)["\']', src))
        names |= set(re.findall(r'["\'](VSE_[A-Z0-9_]+)["\']\s+(?:not\s+)?in\s+os\.environ', src))
    return names


def documented_switches():
    """The bullets under **Environment switches of the product.** in INTEGRATION.md (up to the next blank line)."""
    lines = open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines()
    i = next(k for k, ln in enumerate(lines) if ln.startswith("**Environment switches of the product.**"))
    names = set()
    for ln in lines[i + 1:]:
        if not ln.strip():
            break
        m = re.match(r"- `(VSE_[A-Z0-9_]+)", ln)
        if m:
            names.add(m.group(1))
    return names


def test_library_exports_header(built_lib):
    lib = ctypes.CDLL(built_lib)
    names = declared_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/vse_hip.h but not exported"
    assert set(names) == set(engine.EXPORTS)


def test_record_layouts_and_abi_version_4(built_lib):
    """Record sizes agree between ir.py and the C structs; ABI version 4 (kernel names are read from a record, without a plan)."""
    lib = engine.load_library()
    assert lib.vse_sizeof_op() == ir.OP_DT.itemsize == 352
    assert lib.vse_sizeof_view() == ir.VIEW_DT.itemsize == 40
    assert lib.vse_abi_version() == 4


def test_environment_switches_are_documented():
    """The product reads exactly the documented environment switches: no experiment switch (kernel routing, thresholds, ablations)
    reaches the library or the compiler, and no documented switch is dead."""
    doc = documented_switches()
    assert doc, "no switch list found in INTEGRATION.md"
    assert product_env_reads() == doc


def test_product_refuses_without_gpu(built_lib):
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(engine.VseError):
        engine.Context(0)
