"""CPU test (no GPU) of tests/codeobj.py, the helper the *_codegen tests read the library's code objects with: the notes
parser and the three name-matching modes on a hand-written note, and that the library is unbundled once per process."""
import codeobj

# three kernels as llvm-readelf --notes prints them (abridged): k_pose, one instantiation of the template k_pose<2>, and
# k_pose_refine, whose name has k_pose as a prefix and whose note states no agpr_count and no spill counts
NOTES = """Displaying notes found in: .note
  Owner                Data size 	Description
  AMDGPU               0x00000400	NT_AMDGPU_METADATA (AMDGPU Metadata)
    AMDGPU Metadata:
        ---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 16384
    .max_flat_workgroup_size: 256
    .name:           _ZN12_GLOBAL__N_16k_poseEPKdPd
    .private_segment_fixed_size: 0
    .sgpr_spill_count: 0
    .symbol:         _ZN12_GLOBAL__N_16k_poseEPKdPd.kd
    .vgpr_count:     48
    .vgpr_spill_count: 0
  - .agpr_count:     4
    .group_segment_fixed_size: 0
    .max_flat_workgroup_size: 1024
    .name:           _ZN12_GLOBAL__N_16k_poseILi2EEEvPKdPd
    .private_segment_fixed_size: 24
    .sgpr_spill_count: 3
    .symbol:         _ZN12_GLOBAL__N_16k_poseILi2EEEvPKdPd.kd
    .vgpr_count:     128
    .vgpr_spill_count: 7
  - .args:           []
    .group_segment_fixed_size: 0
    .max_flat_workgroup_size: 64
    .name:           _ZN12_GLOBAL__N_113k_pose_refineEPd
    .private_segment_fixed_size: 0
    .symbol:         _ZN12_GLOBAL__N_113k_pose_refineEPd.kd
    .vgpr_count:     9
  - .name:           _ZN12_GLOBAL__N_16k_poseEPKdPd.kd
    .vgpr_count:     1
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...
"""
PLAIN, TEMPLATE, LONGER = ("_ZN12_GLOBAL__N_16k_poseEPKdPd", "_ZN12_GLOBAL__N_16k_poseILi2EEEvPKdPd",
                           "_ZN12_GLOBAL__N_113k_pose_refineEPd")


def test_notes_parser_and_matching_modes():
    mds = codeobj.parse_notes(NOTES, "obj")
    # an entry whose name ends in .kd is no kernel; the version list's items have no name
    assert [md["name"] for md in mds] == [PLAIN, TEMPLATE, LONGER]
    assert mds[0] == dict(name=PLAIN, object="obj", agpr_count=0, group_segment_fixed_size=16384, max_flat_workgroup_size=256,
                          private_segment_fixed_size=0, sgpr_spill_count=0, vgpr_count=48, vgpr_spill_count=0)
    assert mds[1] == dict(name=TEMPLATE, object="obj", agpr_count=4, group_segment_fixed_size=0, max_flat_workgroup_size=1024,
                          private_segment_fixed_size=24, sgpr_spill_count=3, vgpr_count=128, vgpr_spill_count=7)
    # keys the note does not state are absent, not zero: the callers write md.get("agpr_count", 0) or fail on md[key]
    assert mds[2] == dict(name=LONGER, object="obj", group_segment_fixed_size=0, max_flat_workgroup_size=64,
                          private_segment_fixed_size=0, vgpr_count=9)

    def names(needle, match):
        return [md["name"] for md in codeobj.select(mds, needle, match)]
    assert names("k_pose", "substring") == [PLAIN, TEMPLATE, LONGER]
    assert names("k_pose", "word") == [PLAIN, TEMPLATE, LONGER]       # no digit follows k_pose in any of the three
    assert names("k_pose", "mangled") == [PLAIN]
    assert names("k_poseILi2E", "substring") == [TEMPLATE] and names("k_pose_refine", "mangled") == [LONGER]
    assert names("k_poseILi", "word") == [] and names("k_poseIL", "word") == [TEMPLATE]      # a digit behind the needle
    assert names("k_posf", "substring") == names("k_posf", "word") == names("k_posf", "mangled") == []
    # select hands out copies
    codeobj.select(mds, "k_pose")[0]["vgpr_count"] = -1
    assert mds[0]["vgpr_count"] == 48


def test_library_is_unbundled_once(monkeypatch):
    first = codeobj.code_objects()
    assert first and all("amdgcn" in o for o in first)

    def no_second_run(*a, **kw):
        raise AssertionError("code_objects() started a process again: %r" % (a,))
    monkeypatch.setattr(codeobj.subprocess, "run", no_second_run)
    monkeypatch.setattr(codeobj.L, "build", no_second_run)
    assert codeobj.code_objects() is first
