"""The node agent's C ABI is declared in nodeagent/nodeagent.h and bound in
gpu_provisioner_amd/nodeagent.py (the table ``_ABI`` and the ctypes.Structure
classes). These tests hold the two against each other. All CPU, no GPU:

- layout: a program generated from the Structure classes includes the header,
  is compiled with the host C++ compiler alone (so the header is free of HIP)
  and prints size, offsets and field sizes, and the limits the Python
  constants mirror;
- coverage: the prototypes of the header, parsed from its text, are the keys
  of ``_ABI`` with the same return and parameter types, and every one resolves
  in the built library;
- truncation: 64-bit seeds, indices and pointers passed as plain Python ints
  through the public methods arrive whole (argument checks and pure host code
  only: nothing here touches a device).
"""
import ctypes
import os
import re
import shlex
import shutil
import subprocess

import pytest

from gpu_provisioner_amd import nodeagent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "nodeagent", "nodeagent.h")

STRUCTS = {
    "na_mfma_record": nodeagent.MfmaRecord,
    "na_lds_record": nodeagent.LdsRecord,
    "na_valu_record": nodeagent.ValuRecord,
    "na_memtest_result": nodeagent._MemtestResultC,
    "na_mfma_sweep_result": nodeagent._MfmaSweepResultC,
    "na_lds_sweep_result": nodeagent._LdsSweepResultC,
    "na_valu_sweep_result": nodeagent._ValuSweepResultC,
}

# header macro -> the Python constant that mirrors it
CONSTANTS = {
    "NA_OK": nodeagent.NA_OK,
    "NA_ERR_HIP": nodeagent.NA_ERR_HIP,
    "NA_ERR_VERIFY": nodeagent.NA_ERR_VERIFY,
    "NA_ERR_ARG": nodeagent.NA_ERR_ARG,
    "NA_SWEEP_MAX_LISTED": nodeagent.MFMA_SWEEP_MAX_LISTED,
    "NA_SWEEP_WAVES_PER_WG": nodeagent.MFMA_SWEEP_WAVES_PER_WG,
    "NA_LDS_PHASES": len(nodeagent.LDS_SWEEP_PHASES),
    "NA_LDS_GRANULE": nodeagent.LDS_SWEEP_GRANULE,
    "NA_LDS_MAX_BYTES": nodeagent.LDS_SWEEP_MAX_BYTES,
    "NA_VALU_PHASES": len(nodeagent.VALU_SWEEP_PHASES),
    "NA_VALU_MAX_ITERS": nodeagent.VALU_SWEEP_MAX_ITERS,
}


def _ensure_lib():
    import __graft_entry__ as g

    if not os.path.exists(g.LIB_PATH):
        g.build()
    return g.LIB_PATH


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


# -- layout ---------------------------------------------------------------------


@pytest.fixture(scope="module")
def header_says(tmp_path_factory):
    """What the host compiler makes of the header: {"na_x": sizeof,
    "na_x.field": (offsetof, sizeof), "NA_MACRO": value}."""
    cxx = shlex.split(os.environ.get("CXX", "c++"))
    if shutil.which(cxx[0]) is None:
        pytest.skip(f"no host C++ compiler ({cxx[0]}) to read nodeagent.h with")
    lines = []
    for c_name, cls in STRUCTS.items():
        lines.append(f'printf("{c_name} %zu\\n", sizeof({c_name}));')
        for field, _type in cls._fields_:
            lines.append(f'printf("{c_name}.{field} %zu %zu\\n", offsetof({c_name}, {field}), '
                         f"sizeof((({c_name}*)0)->{field}));")
    for macro in CONSTANTS:
        lines.append(f'printf("{macro} %lld\\n", (long long)({macro}));')
    tmp = tmp_path_factory.mktemp("abi")
    src, exe = tmp / "layout.cpp", tmp / "layout"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"nodeagent.h\"\n"
                   "int main() {\n" + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run(cxx + ["-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    says = {}
    for line in out.splitlines():
        name, *numbers = line.split()
        says[name] = tuple(map(int, numbers)) if len(numbers) > 1 else int(numbers[0])
    return says


def test_every_structure_class_is_checked():
    mirrors = {v for v in vars(nodeagent).values()
               if isinstance(v, type) and issubclass(v, ctypes.Structure)}
    assert mirrors == set(STRUCTS.values())
    assert len(set(STRUCTS.values())) == len(STRUCTS)


@pytest.mark.parametrize("c_name", list(STRUCTS))
def test_structure_layout_matches_header(header_says, c_name):
    cls = STRUCTS[c_name]
    assert ctypes.sizeof(cls) == header_says[c_name]
    for field, _type in cls._fields_:
        descriptor = getattr(cls, field)
        assert (descriptor.offset, descriptor.size) == header_says[f"{c_name}.{field}"], field


def test_constants_match_header(header_says):
    assert {macro: header_says[macro] for macro in CONSTANTS} == CONSTANTS
    assert (nodeagent.MFMA_SWEEP_MAX_LISTED == nodeagent.LDS_SWEEP_MAX_LISTED
            == nodeagent.VALU_SWEEP_MAX_LISTED == 8)


# -- coverage -------------------------------------------------------------------

_SCALARS = {
    "int": ctypes.c_int, "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float,
    "double": ctypes.c_double, "char": ctypes.c_char, "uint32_t": ctypes.c_uint32,
    "uint64_t": ctypes.c_uint64, **STRUCTS,
}


def _ctype(c_type: str):
    """A parameter or return type of the header, spelled in ctypes by the
    rules the binding follows."""
    c_type = c_type.strip()
    if not c_type.endswith("*"):
        return _SCALARS[c_type]
    pointee = c_type[:-1].strip()
    if pointee == "const char":
        return ctypes.c_char_p  # a string the library owns
    pointee = pointee.removeprefix("const ")
    return ctypes.c_void_p if pointee == "void" else ctypes.POINTER(_SCALARS[pointee])


def _prototypes() -> dict:
    """symbol -> (restype, argtypes), from the text of the header."""
    text = open(HEADER).read()
    text = text[text.index('extern "C" {'):]
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    found = {}
    prototype = r"^([\w ]+?\*?) ?\b(na_\w+)\(([^)]*)\);"
    for ret, name, params in re.findall(prototype, text, flags=re.M):
        params = [] if params.strip() == "void" else params.split(",")
        # a parameter is its type and then its name
        argtypes = tuple(_ctype(re.sub(r"\w+\s*$", "", p)) for p in params)
        assert name not in found, name
        found[name] = (_ctype(ret), argtypes)
    return found


def test_table_binds_exactly_the_headers_prototypes():
    header = _prototypes()
    assert len(header) > 40  # the parse found them
    assert set(header) == set(nodeagent._ABI)
    for name, signature in header.items():
        assert nodeagent._ABI[name] == signature, name
    # and no entry point is declared outside the extern "C" block
    assert set(re.findall(r"\bna_\w+(?=\()", open(HEADER).read())) == set(header)


def test_every_prototype_resolves_and_is_bound(cpu_agent):
    raw = ctypes.CDLL(_ensure_lib())
    for name, (restype, argtypes) in nodeagent._ABI.items():
        assert hasattr(raw, name), f"{name} is prototyped but not exported"
        fn = getattr(cpu_agent.lib, name)
        assert (fn.restype, tuple(fn.argtypes)) == (restype, argtypes), name


def test_a_missing_symbol_fails_at_load_with_its_name(monkeypatch):
    _ensure_lib()
    monkeypatch.setitem(nodeagent._ABI, "na_no_such_entry_point", (ctypes.c_int, ()))
    with pytest.raises(nodeagent.NodeAgentError, match="na_no_such_entry_point"):
        nodeagent._load_lib()


# -- truncation -------------------------------------------------------------------

BIG = (1 << 40) + 9  # an unbound call would pass it as the C int 9
M32 = (1 << 32) - 1


@pytest.mark.parametrize("fam", ["mfma", "mx"])
def test_matrix_sweep_expected_takes_64_bit_seed_and_wave(cpu_agent, fam):
    seed, wave, outer = BIG, (1 << 33) + 5, 3
    got = getattr(cpu_agent, f"{fam}_sweep_expected")(wave, outer, seed)
    want = ctypes.c_uint64(0)
    rc = getattr(cpu_agent.lib, f"na_{fam}_sweep_expected")(
        ctypes.c_ulonglong(seed), ctypes.c_ulonglong(wave), outer, ctypes.byref(want))
    assert rc == nodeagent.NA_OK and got == want.value
    # and the high halves matter to the answer
    assert got != getattr(cpu_agent, f"{fam}_sweep_expected")(wave & M32, outer, seed)
    assert got != getattr(cpu_agent, f"{fam}_sweep_expected")(wave, outer, seed & M32)


def test_lds_sweep_expected_takes_64_bit_seed_and_workgroup(cpu_agent):
    # the workgroup enters as workgroup mod C, C = lds_bytes / 1024 chunks; 2^32 is no
    # multiple of C = 20, so the index (mod 20: 18) and its low half (2) differ in rotation
    seed, workgroup, lds_bytes, iters = BIG, (1 << 32) + 2, 20 * 1024, 2
    got = cpu_agent.lds_sweep_expected(workgroup, lds_bytes, iters, seed)
    want = (ctypes.c_uint64 * len(nodeagent.LDS_SWEEP_PHASES))()
    rc = cpu_agent.lib.na_lds_sweep_expected(
        ctypes.c_ulonglong(seed), ctypes.c_ulonglong(workgroup), ctypes.c_longlong(lds_bytes),
        iters, want, len(want))
    assert rc == nodeagent.NA_OK and got == list(want)
    assert got != cpu_agent.lds_sweep_expected(workgroup & M32, lds_bytes, iters, seed)
    assert got != cpu_agent.lds_sweep_expected(workgroup, lds_bytes, iters, seed & M32)


def test_valu_sweep_expected_takes_64_bit_seed_and_wave(cpu_agent):
    seed, wave, iters = BIG, (1 << 33) + 5, 2
    got = cpu_agent.valu_sweep_expected(wave, iters, seed)
    want = (ctypes.c_uint64 * len(nodeagent.VALU_SWEEP_PHASES))()
    rc = cpu_agent.lib.na_valu_sweep_expected(
        ctypes.c_ulonglong(seed), ctypes.c_ulonglong(wave), iters, want)
    assert rc == nodeagent.NA_OK and got == list(want)
    assert got != cpu_agent.valu_sweep_expected(wave & M32, iters, seed)
    assert got != cpu_agent.valu_sweep_expected(wave, iters, seed & M32)


@pytest.mark.parametrize("ptr", [(1 << 40) + 16, 1 << 40])
def test_memtest_calls_take_64_bit_pointers(cpu_agent, ptr):
    """A size that is no multiple of 16 is refused by the argument check, ahead
    of any HIP call, so the pointer is only printed, never followed."""
    assert cpu_agent.memtest_fill(0, ptr, 24) == nodeagent.NA_ERR_ARG
    assert f"na_memtest_fill: pointer {ptr:#x} " in cpu_agent._err()
    assert "bytes (24)" in cpu_agent._err()
    rc, _res = cpu_agent.memtest_verify(0, ptr, (1 << 35) + 8)
    assert rc == nodeagent.NA_ERR_ARG
    assert f"na_memtest_verify: pointer {ptr:#x} " in cpu_agent._err()
    assert f"bytes ({(1 << 35) + 8})" in cpu_agent._err()


@pytest.mark.parametrize("ptr", [(1 << 40) + 16, 1 << 40])
def test_copy_run_takes_64_bit_pointers_and_size(cpu_agent, ptr):
    """Overlapping ranges, a misaligned pointer and a size that is no multiple
    of 16 are refused by the argument check, ahead of any HIP call, so the
    pointers are only printed, never followed."""
    other = ptr + (1 << 33)
    assert cpu_agent.copy_run(0, ptr, ptr + 16, 32) == nodeagent.NA_ERR_ARG
    assert f"na_copy_run: src {ptr:#x} and dst {ptr + 16:#x} overlap" in cpu_agent._err()
    assert cpu_agent.copy_run(0, ptr, other + 8, 32) == nodeagent.NA_ERR_ARG
    assert f"na_copy_run: src {ptr:#x} and dst {other + 8:#x} must be" in cpu_agent._err()
    assert cpu_agent.copy_run(0, ptr, other, (1 << 35) + 8) == nodeagent.NA_ERR_ARG
    assert f"na_copy_run: bytes ({(1 << 35) + 8})" in cpu_agent._err()
