"""What the CPU tests read from libpgx.so's gfx950 code objects and from the compiler's listings, in one place: the unbundled
objects (once per process), the AMDGPU metadata of their kernels (llvm-readelf --notes, once per object), a kernel's
disassembly (llvm-objdump -d, once per object) and the listing of one source file under the library's flags (once per file).
A plain helper module: the *_codegen tests import it."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import photogrammetry_amd._lib as L

LLVM = "/opt/rocm/lib/llvm/bin"
HIPCC = "/opt/rocm/bin/hipcc"
# photogrammetry_amd/csrc/Makefile's code-generation flags, and a device-only listing in place of an object
LISTING_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
                 "--cuda-device-only", "-S"]
KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "max_flat_workgroup_size")
# how a needle selects kernel names.  The callers differ on purpose: "substring" also takes every template instantiation
# and every longer name (k_knn_fp4 -> its four forms); "word" takes the name unless a digit follows (k_ba_lin, not a
# k_ba_lin2); "mangled" takes the length-prefixed identifier followed by E, which is in no other kernel's name and in no
# template instantiation's ("6k_poseE", not k_pose_refine)
MATCH = {
    "substring": lambda needle, name: needle in name,
    "word": lambda needle, name: re.search(needle + r"\D", name + " ") is not None,
    "mangled": lambda needle, name: "%d%sE" % (len(needle), needle) in name,
}

_state = {}


def _tmp():
    if "tmp" not in _state:
        _state["tmp"] = tempfile.mkdtemp(prefix="pgx_codeobj_")
        atexit.register(shutil.rmtree, _state["tmp"], ignore_errors=True)
    return _state["tmp"]


def code_objects():
    """Paths of the amdgcn code objects bundled in libpgx.so (built first), unbundled once per process."""
    if "objects" not in _state:
        if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
            pytest.skip("llvm-readelf / llvm-objdump not found")
        L.build()
        d = os.path.join(_tmp(), "objects")
        os.mkdir(d)
        so = os.path.join(d, "libpgx.so")
        shutil.copy(L.LIB_PATH, so)
        # unbundles next to the copy
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=d, check=True, capture_output=True)
        _state["objects"] = [os.path.join(d, f) for f in sorted(os.listdir(d)) if "amdgcn" in f]
    return _state["objects"]


def parse_notes(notes, obj=None):
    """llvm-readelf --notes text -> [{"name", "object", and each of KEYS the note states}] of its kernels, in the note's
    order.  Kernels are list items that start with "  - .agpr_count:" or "  - .args:"; .kd symbols are skipped."""
    out = []
    for item in re.split(r"\n  - (?=\.)", notes):
        m = re.search(r"\.name:\s+(\S+)", item)
        if not m or m.group(1).endswith(".kd"):
            continue
        md = {"name": m.group(1), "object": obj}
        for key in KEYS:
            mm = re.search(r"\.%s:\s+(\d+)" % key, item)
            if mm:
                md[key] = int(mm.group(1))
        out.append(md)
    return out


def select(mds, needle, match="substring"):
    return [dict(md) for md in mds if MATCH[match](needle, md["name"])]


@functools.lru_cache(maxsize=None)
def _object_kernels(obj):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, capture_output=True,
                           text=True).stdout
    return parse_notes(notes, obj)


def kernels(needle, match="substring"):
    """Metadata dictionaries of every kernel of the library whose name `needle` selects under MATCH[match]."""
    return [md for o in code_objects() for md in select(_object_kernels(o), needle, match)]


@functools.lru_cache(maxsize=None)
def disassembly(obj, *flags):
    return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", *flags, obj], check=True, capture_output=True,
                          text=True).stdout


def kernel_body(md):
    """Disassembly text of the kernel of one metadata dictionary, from its label to s_endpgm."""
    m = re.search(r"<%s>:\n(.*?)s_endpgm" % re.escape(md["name"]), disassembly(md["object"]), flags=re.S)
    assert m, md["name"]
    return m.group(1)


@functools.lru_cache(maxsize=None)
def _library_lines():
    return "\n".join(disassembly(o, "--no-show-raw-insn") for o in code_objects()).splitlines()


def function_lines(needle):
    """Instruction lines (no raw encodings, // comments stripped) of the first function of the library whose symbol contains
    `needle`."""
    out, on = [], False
    for ln in _library_lines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            if on:
                break
            on = needle in m.group(1)
            continue
        if on:
            out.append(re.sub(r"//.*$", "", ln))
    return out


@functools.lru_cache(maxsize=None)
def _listing(source):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = os.path.join(_tmp(), source + ".s")
    subprocess.run([HIPCC, *LISTING_FLAGS, os.path.join(L.CSRC, source), "-o", out], check=True, capture_output=True)
    return open(out).read().split("\n")


def listing(source, needle):
    """(lines, starts): the compiler's listing of csrc/<source> under LISTING_FLAGS and the indices of the labels of the
    functions whose mangled name contains `needle`."""
    lines = _listing(source)
    return lines, [i for i, l in enumerate(lines) if re.match(r"^_ZN.*%s.*:" % needle, l)]


def function_end(lines, start):
    return next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))


def instruction(line):
    """The instruction of one listing line without its comment; None for labels, directives and comment lines."""
    if line.startswith("\t") and not line.startswith("\t.") and not line.strip().startswith(";"):
        return line.strip().split(";")[0].strip()
    return None


def instructions(lines, start):
    """The instructions of the function whose label is lines[start]."""
    return [i for i in map(instruction, lines[start:function_end(lines, start)]) if i is not None]
