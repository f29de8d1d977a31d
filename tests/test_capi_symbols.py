"""The C-ABI library loads and exports every symbol include/copra_hip.h declares (no compute calls: no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(copra_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_boundary():
    names = _declared_functions()
    for must in ("copra_batch_create", "copra_batch_set_system", "copra_batch_solve", "copra_batch_get_results",
                 "copra_batch_dump_qp", "copra_qp_solve_dense_batch", "copra_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in _declared_functions():
        assert hasattr(lib, name), "libcopra_hip.so does not export %s" % name
    lib.copra_abi_version.restype = ctypes.c_int
    assert lib.copra_abi_version() >= 1


def test_no_cpu_fallback_without_a_device():
    """Without a usable HIP device every compute entry point must fail loudly (COPRA_ERR_HIP), never fall back."""
    import numpy as np
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present")
    from copra_amd import BatchLMPC
    with pytest.raises(RuntimeError):
        BatchLMPC(2, 1, 10, 4, [dict(kind="target", M=np.eye(2), p=[0.0, -1.0])], [])


def test_product_package_never_imports_the_oracle_or_emulator():
    """The oracle / emulator are test infrastructure: nothing under copra_amd/ may reference them."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "copra_amd")):
        for f in files:
            if f.endswith((".py", ".hpp", ".hip", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert "pyoracle" not in src and "copra_oracle" not in src and "pyemu" not in src, f
                if f.endswith((".py",)):
                    assert "tests.emu" not in src and "emu_harness" not in src, f


def test_no_matrix_instruction_hazard_across_a_branch(tmp_path):
    """tools/mfma_hazard_lint.py on the SHIPPED binary (its gfx950 code objects extracted and disassembled): no matrix-instruction result
    is read fewer wait states later than the hardware needs on ANY path of the compiled control flow.  Round 4 found the compiler counting
    them on the fall-through side of a wave-uniform branch only -- wrong Riccati factors on the taken side, invisible to the emulator."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import mfma_hazard_lint as lint
    from copra_amd import _capi
    _capi.build_library()
    hits, nobj, nmfma = lint.lint_library(os.path.join(lint.CSRC, "libcopra_hip.so"))
    assert nobj >= 5 and nmfma > 1500  # (the kernels with matrix instructions were really looked at)
    assert not hits, hits[:5]
    # ... and the lint does find the pattern where it exists (the sweep as it was compiled before the fix, reduced to its skeleton)
    tmp = str(tmp_path)
    bad = os.path.join(tmp, "synthetic.s")
    with open(bad, "w") as fh:
        fh.write("copra_synthetic_kernel:\n\tv_mfma_f64_4x4x4_4b_f64 v[28:29], v[28:29], v[10:11], v[32:33]\n\ts_cbranch_vccnz .LBB0_2\n"
                 "\ts_nop 4\n\tv_cndmask_b32_e64 v11, v11, v29, s[12:13]\n\tv_cndmask_b32_e64 v10, v10, v28, s[12:13]\n.LBB0_2:\n"
                 "\tv_mfma_f64_4x4x4_4b_f64 v[30:31], v[22:23], v[28:29], v[2:3]\n\ts_endpgm\n")
    found = lint.lint(bad)
    assert len(found) == 1 and found[0][3] == 8 and found[0][5] == 1 and found[0][6] == 6  # (the reader behind the label, one wait state away)
    dis = os.path.join(tmp, "synthetic.dis")
    with open(dis, "w") as fh:  # the same in llvm-objdump's form: the branch target is an offset
        fh.write("0000000000001000 <copra_synthetic_kernel>:\n"
                 "\tv_mfma_f64_4x4x4_4b_f64 v[28:29], v[28:29], v[10:11], v[32:33] // 000000001000: D3EF001C 0482151C\n"
                 "\ts_cbranch_vccnz 3                                          // 000000001008: BF870003 <copra_synthetic_kernel+0x18>\n"
                 "\ts_nop 4                                                    // 00000000100C: BF800004\n"
                 "\tv_cndmask_b32_e64 v11, v11, v29, s[12:13]                  // 000000001010: D100000B 00323B0B\n"
                 "\tv_mfma_f64_4x4x4_4b_f64 v[30:31], v[22:23], v[28:29], v[2:3] // 000000001018: D3EF001E 040A3916\n"
                 "\ts_endpgm                                                   // 000000001020: BF810000\n")
    found = lint.lint(dis, disassembly=True)
    assert len(found) == 1 and found[0][5] == 1 and found[0][6] == 6


def test_every_engine_option_takes_part_in_the_mode_fuzzer():
    """round-4 verdict, item 6: copra_options_t is the variant surface -- 21 fields since round 5 (37 before) -- and tests/fuzz/fuzz_modes.py
    runs random controllers under every one of them (a 240-controller slice of it is in the GPU suite).  The header's field list, the ctypes
    mirror and the fuzzer's option sets must name the same options."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "fuzz"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import fuzz_modes
    from copra_amd import _capi
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    body = text[text.index("typedef struct {\n    int struct_size;"):text.index("} copra_options_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for m in re.finditer(r"^\s*(?:int|double)\s+([^;]+);", body, flags=re.M):
        fields += [n.strip() for n in m.group(1).split(",")]
    assert fields[0] == "struct_size" and tuple(fields[1:]) == _capi.OPTION_NAMES
    assert len(_capi.OPTION_NAMES) <= 25
    covered = set().union(*[set(o) for o in fuzz_modes.OPTION_SETS])
    assert covered == set(_capi.OPTION_NAMES), (covered ^ set(_capi.OPTION_NAMES))
    assert 240 // 8 >= len(fuzz_modes.OPTION_SETS)  # (the GPU suite's slice reaches every set)


def test_only_the_two_allocator_policies_allocate_or_free():
    """Ownership of device and pinned memory is by type (copra_amd/csrc/device_mem.hpp): hipMalloc / hipFree / hipHostMalloc / hipHostFree
    are called from the two policies in engine.hpp, DeviceMem and PinnedMem, and from nowhere else under copra_amd/csrc."""
    csrc = os.path.join(ROOT, "copra_amd", "csrc")
    calls = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\b")
    found = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".hpp", ".inc", ".h")):
            continue
        for no, line in enumerate(open(os.path.join(csrc, f), errors="replace"), 1):
            found += [(f, no, m.group(1)) for m in calls.finditer(line)]
    assert sorted(c for _, _, c in found) == ["hipFree", "hipHostFree", "hipHostMalloc", "hipMalloc"], found
    assert {f for f, _, _ in found} == {"engine.hpp"}
    text = open(os.path.join(csrc, "engine.hpp")).read()
    dev = text[text.index("struct DeviceMem {"):text.index("struct PinnedMem {")]
    pin = text[text.index("struct PinnedMem {"):]
    pin = pin[:pin.index("};")]
    assert set(calls.findall(dev)) == {"hipMalloc", "hipFree"} and set(calls.findall(pin)) == {"hipHostMalloc", "hipHostFree"}
