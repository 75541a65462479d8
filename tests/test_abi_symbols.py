"""CPU test: libpgx.so builds for gfx950, loads, and exports every symbol include/pgx.h declares; the Python binding's
signature table (_lib.SIGNATURES) says what the header says, and lib() applies it.
No compute call is made (there is no GPU here); creating a context must fail loudly, not fall back."""
import ctypes as C
import os

import numpy as np
import pytest

import photogrammetry_amd._lib as L
from abi_header import HEADER, ROOT, c_prototypes, norm_c


def _declared():
    return sorted(c_prototypes(open(HEADER).read()))


def test_header_and_export_list_agree():
    assert len(_declared()) >= 68
    assert _declared() == sorted(L.EXPORTS)


def ctypes_kind(ctype, ret=False):
    """The ctypes type a C type of pgx.h is declared as in SIGNATURES; an unknown C type is an error."""
    t = norm_c(ctype)
    scalars = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "uint64_t": C.c_uint64, "size_t": C.c_size_t}
    if ret:
        scalars = {"int": C.c_int, "void": None}
    if t in scalars:
        return scalars[t]
    if t == "char*":
        return C.c_char_p
    if t != "void" and t.endswith("*") and t.rstrip("*") in ("void", "int", "int32_t", "uint32_t", "uint16_t", "int64_t", "float",
                                                              "double", "pgx_ctx", "pgx_tracks", "pgx_keypoint", "pgx_pair"):
        return C.c_void_p
    raise AssertionError("test_abi_symbols: no rule for C type %r" % ctype)


def compare(protos, table):
    """List of human-readable mismatches between the header's prototypes and a signature table."""
    bad = []
    for name in sorted(set(protos) | set(table)):
        if name not in protos or name not in table:
            bad.append("%s: %s" % (name, "not in pgx.h" if name in table else "not in SIGNATURES"))
            continue
        (cret, cparams), (restype, argtypes) = protos[name], table[name]
        if restype is not ctypes_kind(cret, ret=True):
            bad.append("%s: returns %s, header says %s" % (name, restype, cret))
        if len(argtypes) != len(cparams):
            bad.append("%s: %d parameters, header has %d" % (name, len(argtypes), len(cparams)))
            continue
        for i, (a, c) in enumerate(zip(argtypes, cparams)):
            if a is not ctypes_kind(c):
                bad.append("%s: parameter %d is %s, header says %r" % (name, i, a, c))
    return bad


def test_signatures_match_the_header():
    protos = c_prototypes(open(HEADER).read())
    assert len(protos) >= 68
    assert compare(protos, L.SIGNATURES) == []
    with pytest.raises(AssertionError):
        ctypes_kind("long double")
    with pytest.raises(AssertionError):
        ctypes_kind("pgx_unknown *")


def test_the_signature_checker_turns_red():
    """A dropped parameter, float <-> double, int <-> pointer and uint64_t -> int must each be reported, naming the export."""
    protos = c_prototypes(open(HEADER).read())

    def mutated(name, change):
        restype, argtypes = L.SIGNATURES[name]
        t = dict(L.SIGNATURES)
        t[name] = (restype, change(list(argtypes)))
        assert t[name] != L.SIGNATURES[name]
        bad = compare(protos, t)
        assert bad and all(b.startswith(name + ":") for b in bad), bad
        return bad

    def swap(i, old, new):
        def change(a):
            assert a[i] is old
            a[i] = new
            return a
        return change
    mutated("pgx_set_detect_params", lambda a: a[:-1])
    mutated("pgx_set_detect_params", swap(1, C.c_float, C.c_double))
    mutated("pgx_triangulate_tracks", swap(8, C.c_double, C.c_float))
    mutated("pgx_match", swap(2, C.c_int, C.c_void_p))
    mutated("pgx_match", swap(1, C.c_void_p, C.c_int))
    mutated("pgx_make_brief_pairs", swap(0, C.c_uint64, C.c_int))
    mutated("pgx_register_frames_dev", swap(19, C.c_uint64, C.c_int))
    t = dict(L.SIGNATURES)
    t["pgx_ctx_destroy"] = (C.c_int, t["pgx_ctx_destroy"][1])
    assert any(b.startswith("pgx_ctx_destroy:") for b in compare(protos, t))
    del t["pgx_version"]
    assert any(b.startswith("pgx_version:") for b in compare(protos, t))


def test_lib_applies_the_table():
    protos = c_prototypes(open(HEADER).read())
    L.build()
    lib = L.lib()
    for name, (_, cparams) in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and len(f.argtypes) == len(cparams), name
        assert list(f.argtypes) == L.SIGNATURES[name][1] and f.restype is L.SIGNATURES[name][0], name
    assert lib.pgx_last_error.restype is C.c_char_p and lib.pgx_version.restype is C.c_char_p
    assert lib.pgx_ctx_destroy.restype is None and lib.pgx_tracks_destroy.restype is None


def test_a_64_bit_seed_survives_as_a_plain_int():
    """Without argtypes the bare int went through as a 32-bit int and the call returned seed 3's table with PGX_OK."""
    import photogrammetry_amd as pg
    from oracle import cref
    L.build()
    seed = 2**40 + 3
    want = cref.gaussian_pairs(seed, 50, 64)
    assert (want != cref.gaussian_pairs(3, 50, 64)).any()
    out = np.zeros((64, 4), dtype=np.int32)
    assert L.lib().pgx_make_brief_pairs(seed, 50, 64, out.ctypes.data) == L.PGX_OK
    assert (out == want).all()
    assert (out != cref.gaussian_pairs(3, 50, 64)).any()
    assert (pg.make_brief_pairs(seed, 50, 64) == want).all()


def test_the_wrong_kind_is_refused_before_the_library_runs():
    L.build()
    with pytest.raises(C.ArgumentError):
        L.lib().pgx_make_brief_pairs(1, 50.5, 64, None)


def test_library_builds_loads_and_exports_everything():
    L.build()
    lib = L.lib()
    for name in _declared():
        assert hasattr(lib, name), name
    assert lib.pgx_version().decode().startswith("pgx")


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import photogrammetry_amd as pg
    with pytest.raises(pg.PgxError):
        pg.Engine(0)


def test_host_helpers_need_no_gpu():
    import numpy as np
    import photogrammetry_amd as pg
    from oracle import cref
    assert (pg.make_brief_pairs(3, 50, 256) == cref.gaussian_pairs(3, 50, 256)).all()
    m = pg.build_dewarp_map(97, 61, [3e-4, 1e-7, 0, 0, 0])
    assert (m == cref.build_distortion_matrix(97, 61, [3e-4, 1e-7, 0, 0, 0])).all()
    with pytest.raises(pg.ArgumentException):
        pg.build_dewarp_map(8, 8, [0.0] * 4)


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under photogrammetry_amd/ may reference it."""
    pkg = os.path.join(ROOT, "photogrammetry_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".hpp", ".inc")) or f == "Makefile":
                text = open(os.path.join(dp, f), errors="ignore").read()
                assert "liboracle" not in text and "pgx_oracle" not in text and "from oracle" not in text \
                    and "import oracle" not in text, os.path.join(dp, f)


def test_missing_rccl_is_an_error_code_not_a_crash():
    """pgx_comm.hip loads librccl at run time; when the file is not there the comm entry points must answer PGX_E_RCCL
    (round 2's loader called dlerror() twice and dereferenced the NULL of the second call).  PGX_RCCL_LIB points the
    loader at one file; a child process, because the loader caches its result for the life of the process."""
    import subprocess
    import sys
    code = ("import ctypes, sys\n"
            "L = ctypes.CDLL(%r)\n"
            "buf = ctypes.create_string_buffer(128)\n"
            "rc1 = L.pgx_comm_unique_id(buf)\n"
            "rc2 = L.pgx_comm_unique_id(buf)\n"
            "print(rc1, rc2)\n" % L.LIB_PATH)
    env = dict(os.environ, PGX_RCCL_LIB="/nonexistent/librccl.so.1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == [str(L.PGX_E_RCCL)] * 2
