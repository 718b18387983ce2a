"""Every C-ABI entry point (`int sv_*(` in include/shotvae_hip.h) is named in at least one GPU test file (tests/*_gpu.py), so a
new entry point cannot ship without a kernel-level test.  The exceptions are listed below, each with its reason: host-only
functions, and entry points reached only through a Python wrapper whose test compares them with a reference."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALLOWED = {
    # host-only: no kernel
    "sv_version": "host-only: ABI number (tests/test_abi_cpu.py)",
    "sv_get_option": "host-only: dispatcher option read (tests/test_abi_cpu.py)",
    "sv_prof_enable": "host-only: in-situ timing switch (bench.py)",
    "sv_prof_tag": "host-only: in-situ timing tag (bench.py)",
    "sv_prof_nested_tag": "host-only: in-situ timing tag (bench.py)",
    "sv_prof_nested_tag_kind": "host-only: in-situ timing tag (bench.py)",
    "sv_prof_collect": "host-only: in-situ timing read-out (bench.py)",
    "sv_debug_wgrad_tile_program": "host-only: schedule table dump (tests/test_abi_cpu.py)",
    "sv_debug_conv_chunk_program": "host-only: schedule table dump (tests/test_abi_cpu.py)",
    # reached through a Python wrapper; the named test compares the result with a reference
    "sv_stream_fork": "engine side-stream fork: tests/test_model_gpu.py::test_step_matches_reference_goldens_fp32",
    "sv_bn_running_update_ex": "engine's deferred running-stat update: tests/test_model_gpu.py::test_step_matches_oracle_b64 "
                               "(running_mean / running_var against the oracle)",
    "sv_repack_strided": "sv_repack is this function with dense strides: every sv_repack of tests/test_kernels_gpu.py",
}


def _declared():
    with open(os.path.join(ROOT, "include", "shotvae_hip.h")) as f:
        return sorted(set(re.findall(r"\bint\s+(sv_\w+)\s*\(", f.read())))


def _gpu_test_text():
    text = ""
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*_gpu.py"))):
        with open(path) as f:
            text += f.read()
    return text


def test_header_parses():
    names = _declared()
    assert len(names) > 50 and "sv_igemm" in names and "sv_smooth_elbo_fwd" in names


def test_every_entry_point_is_named_in_a_gpu_test():
    text = _gpu_test_text()
    missing = [n for n in _declared() if n not in ALLOWED and not re.search(r"\b%s\b" % n, text)]
    assert not missing, "entry points without a kernel-level GPU test (add one, or an allowlist entry with a reason): %s" % missing


def test_allowlist_is_current():
    names = set(_declared())
    stale = [n for n in ALLOWED if n not in names]
    assert not stale, "allowlist entries no longer declared in include/shotvae_hip.h: %s" % stale
    assert all(reason.strip() for reason in ALLOWED.values())


def test_allowlisted_tests_exist():
    """an allowlist entry that names a test names one that exists"""
    for name, reason in ALLOWED.items():
        for path, test in re.findall(r"(tests/\w+\.py)::(\w+)", reason):
            with open(os.path.join(ROOT, path)) as f:
                assert re.search(r"^def %s\(" % test, f.read(), re.M), (name, path, test)
