"""What the CPU tests of the C ABI share (tests/test_abi_units.py and the tests/test_*_abi.py files): the header parsers, the agreement of a unit
of `abi.UNITS` with its headers and the built library, the struct layouts against a C compiler, the one-refusal-per-entry-point loop, and the
metadata notes of a gfx950 code object.  No GPU needed."""
import copy
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile

from extended_legged_gym_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "extended_legged_gym_amd", "csrc")
LIB = os.path.join(CSRC, "liblgstep.so")
HIPCC = "/opt/rocm/bin/hipcc"
LLVM = "/opt/rocm/lib/llvm/bin"


def library(*units):
    """A fresh handle of the built library (its functions carry no prototypes yet) with the named units declared."""
    return abi.declare(C.CDLL(LIB), *units)


def last_error(lib):
    return (lib.lg_mlp_last_error(None) or b"").decode()


# ------------------------------------------------------------------------------------------------------------------------------------- headers
def header_source(header):
    return open(os.path.join(INCLUDE, header)).read()


def header_text(header):
    """A header of include/ without its comments (they speak of other headers' calls)."""
    text = header_source(header)
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_names(*headers):
    """The functions the headers declare, sorted (digits in a name count: `lg_conv_tile_weights_bf16`)."""
    return sorted({n for h in headers for n in re.findall(r"\b(lg_[a-z0-9_]+)\s*\(", header_text(h))})


def header_structs(*headers):
    """The `typedef struct lg_... {` names of the headers, in the headers' order."""
    return [n for h in headers for n in re.findall(r"typedef struct (lg_\w+) \{", header_text(h))]


def unit_structs(unit):
    """name -> ctypes mirror of every struct the unit's headers define."""
    names = header_structs(*abi.UNITS[unit].headers)
    missing = [n for n in names if not (isinstance(getattr(abi, n, None), type) and issubclass(getattr(abi, n), C.Structure))]
    assert not missing, f"{unit}: the headers' typedefs {missing} have no ctypes.Structure of that name in abi.py"
    return {n: getattr(abi, n) for n in names}


# ---------------------------------------------------------------------------------------------------------------------------------- the checks
def check_unit_agreement(unit):
    """The headers' prototypes are the unit's symbols; the library exports each; no other unit's `declare_*` sets one; the unit's own does."""
    names = sorted(abi.symbols(unit))
    assert header_names(*abi.UNITS[unit].headers) == names, (unit, sorted(set(header_names(*abi.UNITS[unit].headers)) ^ set(names)))
    plain = library(*[u for u in abi.UNITS if u != unit])
    for sym in names:
        assert hasattr(plain, sym), f"{sym} is not exported"
        assert getattr(plain, sym).argtypes is None, f"another unit than {unit} declares {sym}"
    fresh = library()
    assert all(getattr(fresh, sym).argtypes is None for sym in names)
    abi.declare(fresh, unit)
    for sym in names:
        assert getattr(fresh, sym).argtypes is not None, sym


def check_struct_layouts(unit, tmp_path):
    """`sizeof` and every `offsetof` as a C compiler lays the unit's headers out, against the ctypes mirrors; every typedef has its mirror."""
    structs = unit_structs(unit)
    if not structs:
        return
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or os.path.join(LLVM, "clang")
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{h}"' for h in abi.UNITS[unit].headers] + ["int main(void) {"]
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / f"layout_{unit}.c", tmp_path / f"layout_{unit}"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", INCLUDE, "-o", str(exe), str(src)], check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, cls in structs.items():
        assert int(got[name]) == C.sizeof(cls), (name, got[name], C.sizeof(cls))
        for field, _ in cls._fields_:
            assert int(got[f"{name}.{field}"]) == getattr(cls, field).offset, (name, field)


def check_refusals(unit, lib, calls, quiet=(), returns_handle=()):
    """`calls`: entry point -> a call the library refuses before it reads a pointer or touches a device.  With `quiet`, the entry points that
    cannot fail or leave no message of their own, they cover the unit; each refused call answers LG_ERR_INVALID (NULL from the entry points
    of `returns_handle`) and leaves a message that starts with its own name."""
    assert set(calls) | set(quiet) == set(abi.symbols(unit)), sorted((set(calls) | set(quiet)) ^ set(abi.symbols(unit)))
    for name, call in calls.items():
        rc = call()
        assert (rc is None or rc == 0) if name in returns_handle else rc == abi.LG_ERR_INVALID, (name, rc)
        assert last_error(lib).startswith(name + ": "), (name, last_error(lib))


# --------------------------------------------------------------------------------------------------------------------------- kernel metadata
def parse_notes(notes):
    """`llvm-readelf --notes` of a code object -> {kernel name: {field: int}} (the numeric fields of its amdhsa.kernels entry)."""
    blocks, cur = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith("- .agpr_count:") or line.startswith("- .args:"):
            cur = {}
        m = re.match(r"-?\s*\.(\w+):\s+(\S+)$", line)
        if m and cur is not None:
            if m.group(1) == "name":
                blocks[m.group(2)] = cur
            elif m.group(2).isdigit():
                cur[m.group(1)] = int(m.group(2))
    return blocks


def object_metadata(obj):
    """The metadata of the gfx950 code object bundled in a host object file; CalledProcessError when a tool refuses it."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}",
                        "--unbundle"], check=True, capture_output=True)
        return parse_notes(subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout)


def kernel_metadata(source, defines=()):
    """{kernel name: {field: int}} of a csrc file cross-compiled for gfx950 with the Makefile's flags (plus `-D` each of `defines`); compiled once
    per process, and every caller gets a copy of its own."""
    return copy.deepcopy(_compiled_metadata(source, tuple(defines)))


@functools.lru_cache(maxsize=None)
def _compiled_metadata(source, defines):
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, os.path.splitext(source)[0] + ".o")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", *[f"-D{x}" for x in defines],
                        "-c", "-o", obj, os.path.join(CSRC, source)], check=True, capture_output=True)
        return object_metadata(obj)


def kernel(blocks, part):
    """The one kernel whose (mangled) name contains `part`."""
    hit = [v for k, v in blocks.items() if part in k]
    assert len(hit) == 1, (part, sorted(blocks))
    return hit[0]


def check_no_spill_no_scratch(blocks, kernels, lds):
    """Each of `kernels` (found by substring) reports no register spill and no scratch, and an LDS size within `lds` (a bound, or kernel -> bound)."""
    for part in kernels:
        r = kernel(blocks, part)
        print(part, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0 and r["private_segment_fixed_size"] == 0, (part, r)
        assert r["group_segment_fixed_size"] <= (lds(part) if callable(lds) else lds), (part, r)
