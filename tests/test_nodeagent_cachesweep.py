"""Chip-wide cache sweep of the node agent (nodeagent/cachesweep.h).

The reference for every checksum is the numpy simulation below, written from
the specification in the header: it builds the memory image of each phase
word by word, walks the 256 threads through their lane-to-address maps and
folds what each would read as the plain recurrence. It shares nothing with
the host code's per-step sums, and known answers pin both.

CPU: exported symbols, the host reference against numpy, the verify and its
attribution of bad workgroups to CUs, phases and an XCD's L2, argument
errors, and check()/report/CLI/chart/docs behaviour against a Python stand-in
for the native library.
GPU (@pytest.mark.gpu, device 0): record checksums of both launches at the
smallest shapes that can go wrong, seed dependence, record sanity, whether
the second launch reads across XCDs, localisation on the GPU's own records
(only HOST data is corrupted; nothing on the GPU is provoked), the default
sweep once, and the end-to-end paths.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

# torch first, before any test loads the agent library: see the note at the
# top of test_nodeagent_memtest.py (one HIP runtime per process — torch's).
try:
    import torch
except ImportError:  # CPU-only environment: the GPU tests cannot run there
    torch = None

from gpu_provisioner_amd import nodeagent
from tests.test_nodeagent_ldssweep import FakeLib as LdsFakeLib
from tests.test_nodeagent_mfmasweep import FakeLib as MfmaFakeLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEED = getattr(nodeagent, "DEFAULT_CACHE_SWEEP_SEED", 0)
PHASES = getattr(nodeagent, "CACHE_SWEEP_PHASES", ())
NPH = 7
U64 = np.uint64
L1_REGION = 16 * 1024
TABLE_WORDS = 4096


def _ensure_lib():
    import __graft_entry__ as g

    if not os.path.exists(g.LIB_PATH):
        g.build()
    return g.LIB_PATH


# ---------------------------------------------------------------------------
# numpy simulation of the specification
# ---------------------------------------------------------------------------


def _mix64(x):
    x = x.copy()
    x ^= x >> U64(30)
    x *= U64(0xBF58476D1CE4E5B9)
    x ^= x >> U64(27)
    x *= U64(0x94D049BB133111EB)
    x ^= x >> U64(31)
    return x


def ref_pattern(seed, pat, g0, words):
    """pat(p, g) for g0 <= g < g0 + words, as uint32."""
    with np.errstate(over="ignore"):
        first = (seed * G + (pat << 40) + g0) & M64
        return (_mix64(U64(first) + np.arange(words, dtype=U64)) >> U64(32)).astype(np.uint32)


T = np.arange(256)
PERM = (T + 67) & 255


def _fold(c, v):
    with np.errstate(over="ignore"):
        return c * U64(G) + v.astype(U64)


def _total(c):
    return int(c.sum(dtype=U64))


def _lo_hi(vec):
    return vec[:, 0] | (vec[:, 1] << U64(32)), vec[:, 2] | (vec[:, 3] << U64(32))


def _read128(mem, c=None, lanes=PERM):
    """One pass: step k has thread t at vector 256k + lanes[t]; lo then hi."""
    c = np.zeros(256, dtype=U64) if c is None else c
    vec = mem.reshape(-1, 4).astype(U64)
    for k in range(len(vec) // 256):
        lo, hi = _lo_hi(vec[256 * k + lanes])
        c = _fold(_fold(c, lo), hi)
    return c


@functools.lru_cache(maxsize=None)
def ref_checksums(seed, workgroup, workgroups, slice_bytes, iters):
    """The seven phase checksums of one workgroup, in the order of PHASES."""
    W = slice_bytes // 4
    C = W // 256
    g0 = workgroup * W
    out = []
    # l1: the leading region, four passes at each polarity, one checksum
    c = None
    for pol in (0, 0xFFFFFFFF):
        mem = ref_pattern(seed, 0, g0, min(slice_bytes, L1_REGION) // 4) ^ np.uint32(pol)
        for _ in range(4):
            c = _read128(mem, c)
    out.append(_total(c))
    # l2: the whole slice, two passes at each polarity
    c = None
    for pol in (0, 0xFFFFFFFF):
        mem = ref_pattern(seed, 1, g0, W) ^ np.uint32(pol)
        for _ in range(2):
            c = _read128(mem, c)
    out.append(_total(c))
    # wt: one pass at each polarity
    c = None
    for pol in (0, 0xFFFFFFFF):
        c = _read128(ref_pattern(seed, 2, g0, W) ^ np.uint32(pol), c)
    out.append(_total(c))
    # atomic: every word receives a from its own thread and a >> 16 from a
    # thread of another wave
    mem = np.zeros(W, dtype=np.uint32)
    a = ref_pattern(seed, 3, g0, W)
    for k in range(C):
        np.add.at(mem, 256 * k + T, a[256 * k + T])
    for k in range(C):
        i = 256 * k + ((T + 64) & 255)
        np.add.at(mem, i, a[i] >> np.uint32(16))
    out.append(_total(_read128(mem)))
    # scalar: each wave folds the whole table from its own start, wrapping
    table = [int(x) for x in ref_pattern(seed, 4, 0, TABLE_WORDS)]
    total = 0
    for v in range(4):
        start = 256 * ((workgroup + v) % 16)
        c = 0
        for j in range(TABLE_WORDS):
            c = (c * G + table[(start + j) % TABLE_WORDS]) & M64
        total += c
    out.append(total & M64)
    # stream: plain 64-bit sums of every lo and hi, pass after pass
    vec = ref_pattern(seed, 5, g0, W).reshape(-1, 4).astype(U64)
    s = np.zeros(256, dtype=U64)
    with np.errstate(over="ignore"):
        for _ in range(iters):
            for k in range(C // 4):
                lo, hi = _lo_hi(vec[256 * k + T])
                s = s + lo + hi
    out.append(_total(s))
    # xread: the neighbour's pattern-5 image
    out.append(_total(_read128(ref_pattern(seed, 5, (workgroup + 1) % workgroups * W, W))))
    return out


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------

SYMBOLS = ("na_cache_sweep_expected", "na_cache_sweep_run", "na_cache_sweep_verify",
           "na_cache_sweep")


def test_library_exports_cache_sweep_symbols():
    lib = ctypes.CDLL(_ensure_lib())
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing symbol {sym}"


def test_constants():
    assert SEED.to_bytes(8, "big") == b"MI355XCS"
    assert PHASES == ("l1", "l2", "wt", "atomic", "scalar", "stream", "xread")
    assert len(PHASES) == NPH
    assert nodeagent.CACHE_SWEEP_GRANULE == 4096
    assert nodeagent.CACHE_SWEEP_MAX_BYTES == 1 << 20
    assert nodeagent.CACHE_SWEEP_TABLE_WORDS == TABLE_WORDS
    # a plain class over the LDS sweep's structs, which the ABI test pins
    assert not issubclass(nodeagent.CacheSweepResult, ctypes.Structure)
    with open(os.path.join(ROOT, "nodeagent", "nodeagent.h")) as f:
        header = f.read()
    for macro in ("NA_CACHE_PHASES 7", "NA_CACHE_GRANULE 4096", "NA_CACHE_MAX_BYTES (1 << 20)",
                  "NA_CACHE_TABLE_WORDS 4096"):
        assert f"#define {macro}" in header, macro


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


# (seed, workgroup, workgroups, slice_bytes, iters)
KNOWN = [
    (0, 0, 1, 4096, 1,
     ["0x9f2a2275ab2ebe80", "0x9fcb43d0bf9874a0", "0x930ff9e65f6a9328", "0xc40767b2653749bc",
      "0xec6984187d6a192c", "0x251f815991426674", "0xaa07bb68baaab87c"]),
    (7, 2, 3, 12288, 2,
     ["0x7fdcb9e1b06dd600", "0x0a085cb6b250c180", "0x622fb7fd688be060", "0x4f92efd6c88d532d",
      "0x56604f7824aec61c", "0x8b1ea07fe5b7fe40", "0xce92965b419ce2d4"]),
    (SEED, 8, 9, 65536, 5,
     ["0x27f9e62fbf137a00", "0x9745dfb481322600", "0xd3a0ded19deb5900", "0x5ecbe64898bfa8b4",
      "0x8ed14b3574459590", "0x101d75fb63856b82", "0xb99a282d247a61e8"]),
]


@pytest.mark.parametrize("seed,workgroup,workgroups,slice_bytes,iters,want", KNOWN)
def test_reference_known_answers(cpu_agent, seed, workgroup, workgroups, slice_bytes, iters, want):
    got = ref_checksums(seed, workgroup, workgroups, slice_bytes, iters)
    assert [f"{x:#018x}" for x in got] == want
    assert cpu_agent.cache_sweep_expected(workgroup, workgroups, slice_bytes, iters, seed) == got


@pytest.mark.parametrize("seed", [0, 7, SEED])
@pytest.mark.parametrize("slice_bytes", [4096, 12288, 65536])
def test_expected_checksums_match_reference(cpu_agent, seed, slice_bytes):
    for workgroups in (1, 3, 9):
        for workgroup in sorted({0, min(1, workgroups - 1), workgroups - 1}):
            for iters in (1, 2, 5):
                want = ref_checksums(seed, workgroup, workgroups, slice_bytes, iters)
                got = cpu_agent.cache_sweep_expected(workgroup, workgroups, slice_bytes, iters,
                                                     seed)
                assert got == want, (workgroups, workgroup, iters,
                                     [PHASES[p] for p in range(NPH) if got[p] != want[p]])


def test_reference_depends_on_seed_workgroup_workgroups_and_iters():
    a = ref_checksums(SEED, 1, 9, 12288, 2)
    assert all(x != y for x, y in zip(a, ref_checksums(SEED + 1, 1, 9, 12288, 2)))
    # every word carries its global index, and the table's start moves
    assert all(x != y for x, y in zip(a, ref_checksums(SEED, 2, 9, 12288, 2)))
    # the number of workgroups enters only where the neighbour wraps
    assert ref_checksums(SEED, 1, 3, 12288, 2) == a
    b = ref_checksums(SEED, 1, 2, 12288, 2)
    assert a[:6] == b[:6] and a[6] != b[6]
    # xread of w is one pass over what w + 1 streams: other checksums, same data
    assert a[6] != ref_checksums(SEED, 2, 9, 12288, 2)[5]
    c = ref_checksums(SEED, 1, 9, 12288, 3)
    assert a[:5] == c[:5] and a[5] != c[5] and a[6] == c[6]


def test_expected_takes_64_bit_seed_and_workgroup(cpu_agent):
    big = (1 << 40) + 9
    got = cpu_agent.cache_sweep_expected(big, big + 1, 4096, 1, big)
    assert got == ref_checksums(big, big, big + 1, 4096, 1)
    assert got != cpu_agent.cache_sweep_expected(9, big + 1, 4096, 1, big)
    assert got != cpu_agent.cache_sweep_expected(big, big + 1, 4096, 1, 9)


def test_expected_argument_errors(cpu_agent):
    out = (ctypes.c_uint64 * NPH)()
    for wg, wgs, slice_bytes, iters, ptr, n in [
            (0, 1, 0, 1, out, NPH), (0, 1, 4095, 1, out, NPH), (0, 1, 2048, 1, out, NPH),
            (0, 1, (1 << 20) + 4096, 1, out, NPH), (0, 1, -4096, 1, out, NPH),
            (0, 1, 4096, 0, out, NPH), (0, 1, 4096, 1, None, NPH), (0, 1, 4096, 1, out, NPH - 1),
            (0, 0, 4096, 1, out, NPH), (3, 3, 4096, 1, out, NPH)]:
        rc = cpu_agent.lib.na_cache_sweep_expected(1, wg, wgs, slice_bytes, iters, ptr, n)
        assert rc == nodeagent.NA_ERR_ARG, (wg, wgs, slice_bytes, iters, n)
        assert "na_cache_sweep_expected" in cpu_agent._err()


def _unit_of(wg):
    """A made-up placement: workgroups 2j and 2j+1 on one CU."""
    u = wg // 2
    return (u % 8, (u // 8) % 4, (u // 32) % 2, (u // 64) % 16)


SLICE, ITERS = 12288, 2


def _records(n, slice_bytes=SLICE, iters=ITERS, seed=SEED):
    """Both launches of n workgroups: 2n records. Launch B runs workgroup w on
    the CU launch A ran workgroup w + 2 on."""
    recs = (nodeagent.LdsRecord * (2 * n))()
    for i in range(2 * n):
        r, w = recs[i], i % n
        want = ref_checksums(seed, w, n, slice_bytes, iters)
        r.checksum[:] = (want[:6] + [0, 0]) if i < n else ([0] * 6 + [want[6], 0])
        r.bad_words, r.first_bad_offset, r.xor_mask = 0, nodeagent.NO_BAD_OFFSET, 0
        r.bad_phase = 0xFFFFFFFF
        # launch A: 30, 31, ... bytes per clock; launch B: a short phase
        r.cycles = iters * slice_bytes // (30 + w) if i < n else 900
        r.realtime, r.workgroup = (10, w) if i < n else (1, w)
        r.xcc, r.se, r.sh, r.cu = _unit_of(w if i < n else (w + 2) % n)
    return recs


def test_verify_clean_records(cpu_agent):
    recs = _records(12)
    rc, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert rc == nodeagent.NA_OK and res.ok, cpu_agent._err()
    assert isinstance(res, nodeagent.CacheSweepResult)
    assert (res.workgroups, res.bad_workgroups, res.units_seen, res.bad_units) == (12, 0, 6, 0)
    assert res.first_bad_workgroup == nodeagent.NO_BAD_WORKGROUP and res.bad_cus == []
    assert res.first_bad_phase == "" and res.first_bad_offset == nodeagent.NO_BAD_OFFSET
    # the same records do not verify under other passes, another seed or size
    assert cpu_agent.cache_sweep_verify(recs, SLICE, 3)[1].first_bad_phase == "stream"
    assert cpu_agent.cache_sweep_verify(recs, SLICE, ITERS, SEED + 1)[1].bad_workgroups == 12
    assert cpu_agent.cache_sweep_verify(recs, 4096, ITERS)[0] == nodeagent.NA_ERR_VERIFY


def test_verify_rate_statistics_come_from_launch_a(cpu_agent):
    recs = _records(12)
    rates = sorted(ITERS * SLICE / recs[i].cycles for i in range(12))
    _, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert res.median_bytes_per_clk == pytest.approx(rates[6], rel=1e-12)
    assert res.min_bytes_per_clk == pytest.approx(rates[0], rel=1e-12)
    assert res.max_bytes_per_clk == pytest.approx(rates[-1], rel=1e-12)
    assert 29.9 < rates[0] < 31 and 40 < rates[-1] < 43
    mhz = sorted(recs[i].cycles / 10 * 100.0 for i in range(12))
    assert res.clock_mhz == pytest.approx(mhz[6], rel=1e-12)


@pytest.mark.parametrize("phase", range(NPH))
def test_verify_one_flipped_bit_names_the_phase(cpu_agent, phase):
    n = 12
    recs = _records(n)
    wg = 3 + phase
    i = wg + n if phase == 6 else wg  # xread is launch B's
    recs[i].checksum[phase] ^= 1 << (phase * 9)
    unit = (recs[i].xcc, recs[i].se, recs[i].sh, recs[i].cu)
    rc, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
    assert (res.bad_workgroups, res.bad_units, res.first_bad_workgroup) == (1, 1, wg)
    assert res.first_bad_phase == PHASES[phase] and res.bad_cus == [unit]
    assert res.first_bad_offset == nodeagent.NO_BAD_OFFSET
    err = cpu_agent._err()
    assert f"cache sweep: 1 of {n} workgroups wrong on 1 CU(s), first workgroup {wg} in phase " \
        f"{PHASES[phase]} on {nodeagent.mfma_unit_name(unit)}" in err
    assert "suspect" not in err
    assert PHASES[phase] in res.describe() and nodeagent.mfma_unit_name(unit) in res.describe()
    # an xread failure also names who wrote the slice: workgroup wg + 1 of launch A
    writer = f"its slice was written by workgroup {wg + 1} on " \
        f"{nodeagent.mfma_unit_name(_unit_of(wg + 1))}"
    assert (writer in err) == (phase == 6)


def test_verify_xread_writer_wraps_around(cpu_agent):
    n = 12
    recs = _records(n)
    recs[2 * n - 1].checksum[6] ^= 1
    rc, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY and res.first_bad_workgroup == n - 1
    assert f"written by workgroup 0 on {nodeagent.mfma_unit_name(_unit_of(0))}" in cpu_agent._err()


def test_verify_record_in_the_wrong_place_is_bad(cpu_agent):
    for launch in (0, 1):
        recs = _records(12)
        recs[12 * launch + 5].workgroup = 4
        rc, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
        assert rc == nodeagent.NA_ERR_VERIFY
        assert (res.bad_workgroups, res.first_bad_workgroup, res.first_bad_phase) == (1, 5, "index")
        assert "phase index" in cpu_agent._err()


def test_verify_a_checksum_that_must_be_zero_is_bad(cpu_agent):
    n = 12
    # launch A carries no xread, launch B nothing but xread; the eighth is unused
    for i, slot, phase in [(4, 6, "xread"), (n + 4, 2, "wt"), (n + 4, 5, "stream"),
                           (4, 7, "index"), (n + 4, 7, "index")]:
        recs = _records(n)
        recs[i].checksum[slot] = 1
        rc, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
        assert rc == nodeagent.NA_ERR_VERIFY, (i, slot)
        assert (res.bad_workgroups, res.first_bad_workgroup, res.first_bad_phase) == (1, 4, phase)
    # and the reference's value in the other launch's slot is as wrong as any
    recs = _records(n)
    recs[4].checksum[6] = ref_checksums(SEED, 4, n, SLICE, ITERS)[6]
    assert cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)[0] == nodeagent.NA_ERR_VERIFY


def test_verify_in_kernel_bad_count_with_correct_checksums_is_bad(cpu_agent):
    recs = _records(12)
    r = recs[7]
    r.bad_words, r.first_bad_offset, r.xor_mask, r.bad_phase = 2, 0x2A40, 0x00010000, 1
    rc, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_workgroups, res.first_bad_workgroup, res.first_bad_phase) == (1, 7, "l2")
    assert (res.bad_words, res.first_bad_offset, res.xor_mask) == (2, 0x2A40, 0x00010000)
    err = cpu_agent._err()
    assert "in phase l2 on " + nodeagent.mfma_unit_name(_unit_of(7)) in err
    assert "2 bad words, first at slice offset 0x2a40, failing bits 0x00010000" in err
    assert "LDS" not in err and "bank" not in err
    assert "first at slice offset 0x2a40, failing bits 0x00010000" in res.describe()
    # the triple belongs to its own phase: an earlier failing phase reports none
    recs[7].checksum[0] ^= 1
    _, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert res.first_bad_phase == "l1" and res.first_bad_offset == nodeagent.NO_BAD_OFFSET
    # launch B's diagnosis is xread's
    recs = _records(12)
    r = recs[12 + 3]
    r.bad_words, r.first_bad_offset, r.xor_mask, r.bad_phase = 1, 0x10, 0x80, 6
    _, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert (res.first_bad_workgroup, res.first_bad_phase, res.first_bad_offset) == (3, "xread", 0x10)


def test_verify_two_workgroups_of_one_cu_are_one_unit(cpu_agent):
    recs = _records(12)
    recs[4].checksum[0] ^= 2
    recs[5].checksum[4] ^= 1 << 40
    rc, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_workgroups, res.bad_units, res.first_bad_workgroup) == (2, 1, 4)
    assert res.bad_cus == [_unit_of(4)] and res.first_bad_phase == "l1"
    recs[10].checksum[0] ^= 1
    _, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert (res.bad_workgroups, res.bad_units) == (3, 2)
    # a workgroup wrong in both launches is one workgroup
    recs[12 + 4].checksum[6] ^= 1
    _, res = cpu_agent.cache_sweep_verify(recs, SLICE, ITERS)
    assert res.bad_workgroups == 3


def test_verify_lists_a_bounded_number_of_cus(cpu_agent):
    n = 2 * (nodeagent.LDS_SWEEP_MAX_LISTED + 2)
    recs = _records(n, 4096, 1)
    for i in range(n):
        recs[i].checksum[4] ^= 1
    _, res = cpu_agent.cache_sweep_verify(recs, 4096, 1)
    assert (res.bad_workgroups, res.bad_units) == (n, n // 2)
    assert res.bad_cus == [_unit_of(2 * i) for i in range(nodeagent.LDS_SWEEP_MAX_LISTED)]
    assert ", ...;" in res.describe()


def test_verify_failures_across_one_xcc_suspect_its_l2(cpu_agent):
    n = 40
    assert _unit_of(2)[0] == _unit_of(18)[0] == _unit_of(34)[0] == 1
    assert len({_unit_of(2), _unit_of(18), _unit_of(34)}) == 3

    def verdict(bad):
        recs = _records(n, 4096, 1)
        for i, phase in bad:
            recs[i].checksum[phase] ^= 1
        rc, res = cpu_agent.cache_sweep_verify(recs, 4096, 1)
        assert rc == nodeagent.NA_ERR_VERIFY and res.bad_workgroups == len(bad)
        return cpu_agent._err(), res

    # l2 and wt on two CUs of xcc1, and an xread whose reader sits on a third
    # (launch B's workgroup 32 runs where launch A's 34 did)
    err, res = verdict([(2, 1), (18, 2), (n + 32, 6)])
    assert "wrong on 3 CU(s), first workgroup 2 in phase l2" in err
    assert "the 3 CUs that failed in a phase the L2 serves are all on xcc1: suspect its L2" in err
    assert "all on xcc1: suspect its L2" in res.describe()
    assert nodeagent.mfma_unit_name(_unit_of(18)) not in res.describe()
    # one CU alone is that CU's business
    err, res = verdict([(2, 1), (3, 3)])
    assert "suspect" not in err and "suspect" not in res.describe()
    # two XCCs: no single L2 explains it
    err, res = verdict([(2, 1), (4, 1)])
    assert "suspect" not in err and "suspect" not in res.describe()
    assert nodeagent.mfma_unit_name(_unit_of(4)) in res.describe()
    # phases that never reach the L2 do not point at it
    err, res = verdict([(2, 0), (18, 4)])
    assert "suspect" not in err and "suspect" not in res.describe()
    # and they do not excuse the ones that do
    err, _ = verdict([(2, 5), (18, 3), (4, 0)])
    assert "the 2 CUs that failed in a phase the L2 serves are all on xcc1: suspect its L2" in err


def test_verify_unwritten_records_are_bad(cpu_agent):
    recs = (nodeagent.LdsRecord * 8)()
    ctypes.memset(recs, 0xFF, ctypes.sizeof(recs))
    rc, res = cpu_agent.cache_sweep_verify(recs, 4096, 1)
    assert rc == nodeagent.NA_ERR_VERIFY and res.bad_workgroups == 4 and res.workgroups == 4
    # the second launch alone missing
    recs = _records(4, 4096, 1)
    ctypes.memset(ctypes.byref(recs, 4 * ctypes.sizeof(nodeagent.LdsRecord)), 0xFF,
                  4 * ctypes.sizeof(nodeagent.LdsRecord))
    rc, res = cpu_agent.cache_sweep_verify(recs, 4096, 1)
    assert rc == nodeagent.NA_ERR_VERIFY and res.bad_workgroups == 4


def test_argument_errors_before_any_hip_call(cpu_agent):
    lib = cpu_agent.lib
    recs = (nodeagent.LdsRecord * 8)()
    ms, gbs = ctypes.c_double(0), ctypes.c_double(0)
    res = nodeagent._LdsSweepResultC()
    big = 1 << 40

    def run(workgroups, slice_bytes, iters, out, n_out):
        return lib.na_cache_sweep_run(0, workgroups, slice_bytes, iters, SEED, out, n_out,
                                      ctypes.byref(ms))

    for args in [(0, 4096, 1, recs, 8), (-2, 4096, 1, recs, 8), ((1 << 20) + 1, 4096, 1, recs, big),
                 (2, 0, 1, recs, 8), (2, 4095, 1, recs, 8), (2, 2048, 1, recs, 8),
                 (2, -4096, 1, recs, 8), (2, (1 << 20) + 4096, 1, recs, 8), (2, 4096, 0, recs, 8),
                 (2, 4096, -1, recs, 8), (2, 4096, (1 << 22) + 1, recs, 8),
                 (2, 4096, 1, None, 8), (2, 4096, 1, recs, 3), (4, 4096, 1, recs, 7),
                 # more than 4 GiB in all
                 (4097, 1 << 20, 1, recs, big), (1 << 20, 8192, 1, recs, big)]:
        assert run(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_cache_sweep_run" in cpu_agent._err()

    def verify(r, n, slice_bytes, iters, out):
        return lib.na_cache_sweep_verify(r, n, slice_bytes, iters, SEED, out)

    for args in [(None, 4, 4096, 1, ctypes.byref(res)), (recs, 0, 4096, 1, ctypes.byref(res)),
                 (recs, 3, 4096, 1, ctypes.byref(res)), (recs, 7, 4096, 1, ctypes.byref(res)),
                 (recs, -2, 4096, 1, ctypes.byref(res)),
                 (recs, 4, 0, 1, ctypes.byref(res)), (recs, 4, 6144, 1, ctypes.byref(res)),
                 (recs, 4, (1 << 20) + 4096, 1, ctypes.byref(res)),
                 (recs, 4, 4096, 0, ctypes.byref(res)), (recs, 4, 4096, 1, None)]:
        assert verify(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_cache_sweep_verify" in cpu_agent._err()
    assert cpu_agent.cache_sweep_verify((nodeagent.LdsRecord * 3)(), 4096, 1)[0] == \
        nodeagent.NA_ERR_ARG

    def sweep(workgroups, slice_bytes, iters, out):
        return lib.na_cache_sweep(0, workgroups, slice_bytes, iters, SEED, out, ctypes.byref(gbs))

    for args in [(-1, 0, 0, ctypes.byref(res)), ((1 << 20) + 1, 0, 0, ctypes.byref(res)),
                 (0, 100, 0, ctypes.byref(res)), (0, (1 << 20) + 4096, 0, ctypes.byref(res)),
                 (0, 0, -1, ctypes.byref(res)), (0, 0, (1 << 22) + 1, ctypes.byref(res)),
                 (0, 0, 0, None), (4097, 1 << 20, 0, ctypes.byref(res))]:
        assert sweep(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_cache_sweep:" in cpu_agent._err()
    with pytest.raises(nodeagent.NodeAgentError):
        cpu_agent.cache_sweep_run(0, workgroups=0)


# -- check() against a Python stand-in library --------------------------------

SICK = [(5, 2, 1, 9), (5, 0, 0, 3)]


class FakeLib(LdsFakeLib):
    """The LDS sweep's stand-in plus na_cache_sweep. ``cache``: {dev: "sick" |
    "slow" | "fewer"}; default clean. A sick GPU has two CUs of one XCC whose
    workgroups fail in the l2 phase."""

    def __init__(self, ngpu=1, cache=None, **kw):
        super().__init__(ngpu=ngpu, **kw)
        self.cache_calls = []
        cache = cache or {}

        def na_cache_sweep(dev, workgroups, slice_bytes, iters, seed, res, gbs):
            self.cache_calls.append((dev, workgroups, slice_bytes.value, iters, seed.value))
            kind = cache.get(dev, "ok")
            r = res._obj
            r.workgroups, r.units_seen, r.clock_mhz = 1024, 255 if kind == "fewer" else 256, 2391.7
            r.bad_workgroups, r.bad_units, r.listed = 0, 0, 0
            r.first_bad_workgroup = nodeagent.NO_BAD_WORKGROUP
            r.first_bad_offset, r.first_bad_phase = nodeagent.NO_BAD_OFFSET, 0xFFFFFFFF
            r.median_bytes_per_clk, r.min_bytes_per_clk, r.max_bytes_per_clk = 31.3, 28.266, 33.0
            gbs._obj.value = 12.34 if kind == "slow" else 19251.16
            if kind != "sick":
                return 0
            r.bad_workgroups, r.bad_units, r.first_bad_workgroup, r.listed = 8, 2, 77, 2
            r.first_bad_phase = 1
            r.bad_words, r.first_bad_offset, r.xor_mask = 53, 0x1F80, 0x00000400
            for k, unit in enumerate(SICK):
                r.bad_list[k][:] = unit
            r.first_bad_unit[:] = SICK[0]
            return nodeagent.NA_ERR_VERIFY

        self.na_cache_sweep = na_cache_sweep


def _agent(monkeypatch, **kw):
    fake = FakeLib(**kw)
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fake)
    return nodeagent.NodeAgent(), fake


def _sweep_fields(g):
    return (g.cache_sweep_gbs, g.cache_sweep_min_cu_bytes_per_clk, g.cache_sweep_units_seen,
            g.cache_sweep_bad_workgroups)


def test_check_default_never_runs_sweep(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check()
    assert fake.cache_calls == [] and fake.lds_calls == [] and fake.sweep_calls == []
    assert report.healthy, report.problems
    assert _sweep_fields(report.gpus[0]) == (0.0, 0.0, 0, 0)
    assert _sweep_fields(nodeagent.GPUReport(index=0)) == (0.0, 0.0, 0, 0)
    # the other sweeps' flags do not reach it
    assert agent.check(lds_sweep=True).healthy and fake.cache_calls == []
    # the stand-ins of the other sweeps' tests have no cache sweep at all
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: LdsFakeLib())
    assert nodeagent.NodeAgent().check(lds_sweep=True).healthy
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: MfmaFakeLib())
    assert nodeagent.NodeAgent().check().healthy


def test_check_clean_sweep_populates_fields(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_CACHE_SWEEP_GBS", 10000.0)
    agent, fake = _agent(monkeypatch)
    report = agent.check(cache_sweep=True)
    assert fake.cache_calls == [(0, 0, 0, 0, SEED)]
    assert fake.lds_calls == [] and fake.sweep_calls == []
    g = report.gpus[0]
    assert report.healthy and g.healthy, report.problems
    assert _sweep_fields(g) == (19251.2, 28.27, 256, 0)
    assert nodeagent.node_condition_from_report(report)["status"] == "True"


def test_check_units_seen_below_cus_is_reported_not_a_problem(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_CACHE_SWEEP_GBS", 10000.0)
    agent, _ = _agent(monkeypatch, cache={0: "fewer"})
    report = agent.check(cache_sweep=True)
    assert report.gpus[0].cache_sweep_units_seen == 255 < report.gpus[0].cus
    assert report.healthy, report.problems


def test_check_eight_gpus_one_sick_l2(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_CACHE_SWEEP_GBS", 10000.0)
    agent, fake = _agent(monkeypatch, ngpu=8, cache={3: "sick"})
    report = agent.check(expect_gpus=8, cache_sweep=True)
    assert [c[0] for c in fake.cache_calls] == list(range(8))
    assert report.problems == [
        "gpu3: cache sweep: 8 of 1024 workgroups wrong on 2 CU(s): all on xcc5: suspect its L2; "
        "first in phase l2, 53 bad words, first at slice offset 0x1f80, failing bits 0x00000400"
    ]
    assert not report.healthy
    assert [g.healthy for g in report.gpus] == [i != 3 for i in range(8)]
    assert [g.cache_sweep_bad_workgroups for g in report.gpus] == [8 * (i == 3) for i in range(8)]
    assert nodeagent.node_condition_from_report(report)["status"] == "False"


def test_check_low_rate_flags_a_problem(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_CACHE_SWEEP_GBS", 10000.0)
    agent, _ = _agent(monkeypatch, cache={0: "slow"})
    report = agent.check(cache_sweep=True)
    assert report.gpus[0].problems == ["cache sweep: 12.3 GB/s below floor 10000.0"]
    assert not report.healthy
    agent, _ = _agent(monkeypatch)
    assert agent.check(cache_sweep=True).healthy


def test_floor_is_derived_from_the_profile():
    """0.70 x the median of the profile's per-process figures."""
    with open(os.path.join(ROOT, "profiles", "cache_sweep_mi355x.txt")) as f:
        runs = [float(x) for line in f if line.startswith("gbs ") for x in line.split()[1:]]
    assert len(runs) >= 5
    assert nodeagent.MIN_CACHE_SWEEP_GBS > 0
    assert nodeagent.MIN_CACHE_SWEEP_GBS == pytest.approx(0.70 * float(np.median(runs)), abs=0.06)


def test_cli_flag_reaches_check(monkeypatch, capsys):
    monkeypatch.setattr(nodeagent, "MIN_CACHE_SWEEP_GBS", 10000.0)
    _, fake = _agent(monkeypatch)
    assert nodeagent.main(["--cache-sweep"]) == 0
    assert [c[0] for c in fake.cache_calls] == [0] and fake.lds_calls == []
    assert json.loads(capsys.readouterr().out)["gpus"][0]["cache_sweep_units_seen"] == 256
    _, fake = _agent(monkeypatch)
    assert nodeagent.main([]) == 0
    assert fake.cache_calls == []
    capsys.readouterr()


def test_chart_passes_cache_sweep_only_when_true():
    import yaml

    chart = os.path.join(ROOT, "charts", "gpu-provisioner-amd")
    with open(os.path.join(chart, "values.yaml")) as f:
        values = yaml.safe_load(f)
    assert values["nodeAgent"]["cacheSweep"] is False
    with open(os.path.join(chart, "templates", "amd-gpu-node-stack.yaml")) as f:
        text = f.read()
    start = text.index("{{- if .Values.nodeAgent.cacheSweep }}")
    end = text.index("{{- end }}", start)
    assert "--cache-sweep \\" in text[start:end]
    assert text.count("--cache-sweep") == 1  # nowhere outside the guard


def test_docs_cover_every_new_report_field():
    with open(os.path.join(ROOT, "docs", "METRICS.md")) as f:
        metrics = f.read()
    for name in ("cache_sweep_gbs", "cache_sweep_min_cu_bytes_per_clk", "cache_sweep_units_seen",
                 "cache_sweep_bad_workgroups"):
        assert name in metrics, name
        assert hasattr(nodeagent.GPUReport(index=0), name)
    for doc in ("DESIGN.md", "OPERATIONS.md"):
        with open(os.path.join(ROOT, "docs", doc)) as f:
            assert "--cache-sweep" in f.read(), doc
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "--cache-sweep" in f.read()


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


_runs = {}


def _run(agent, workgroups, slice_bytes, iters, seed=SEED):
    """One pair of launches per distinct shape, shared by the tests; read-only."""
    key = (workgroups, slice_bytes, iters, seed)
    if key not in _runs:
        torch.cuda.synchronize()
        _runs[key] = agent.cache_sweep_run(0, workgroups, slice_bytes, iters, seed)[0]
    return _runs[key]


_sweeps = []


def _default_sweep(agent):
    if not _sweeps:
        torch.cuda.synchronize()
        _sweeps.append(agent.cache_sweep(0))
    return _sweeps[0]


def _assert_records_match(recs, workgroups, slice_bytes, iters, seed):
    assert len(recs) == 2 * workgroups
    for i, r in enumerate(recs):
        wg = i % workgroups
        want = ref_checksums(seed, wg, workgroups, slice_bytes, iters)
        want = (want[:6] + [0, 0]) if i < workgroups else ([0] * 6 + [want[6], 0])
        got = list(r.checksum)
        print(f"launch {i // workgroups} workgroup {wg} of {slice_bytes} bytes:",
              [f"{x:#x}" for x in got])
        assert got == want, [(PHASES + ("unused",))[p] for p in range(8) if got[p] != want[p]]


SHAPES = [
    (1, 4096, 1),    # one 16-byte access per thread, xread on its own slice
    (3, 12288, 2),   # several steps, an l1 region under 16 KiB, the neighbour's wrap-around
    (9, 65536, 1),   # the l1 region a strict part of the slice, 8 wraps to 0, writers on other XCDs
]


@pytest.mark.gpu
@pytest.mark.parametrize("workgroups,slice_bytes,iters", SHAPES)
def test_gpu_record_checksums_match_reference(agent, workgroups, slice_bytes, iters):
    _assert_records_match(_run(agent, workgroups, slice_bytes, iters), workgroups, slice_bytes,
                          iters, SEED)


@pytest.mark.gpu
def test_gpu_seed_changes_every_phase(agent):
    recs = _run(agent, 3, 12288, 2)
    other = _run(agent, 3, 12288, 2, seed=7)
    _assert_records_match(other, 3, 12288, 2, 7)
    for wg in range(3):
        assert all(a != b for a, b in zip(recs[wg].checksum[:6], other[wg].checksum[:6]))
        assert recs[3 + wg].checksum[6] != other[3 + wg].checksum[6]


@pytest.mark.gpu
def test_gpu_record_sanity(agent):
    recs = _run(agent, 9, 65536, 1)
    assert [r.workgroup for r in recs] == list(range(9)) * 2
    for i, r in enumerate(recs):
        assert r.xcc < 8 and r.se < 4 and r.sh < 2 and r.cu < 16
        assert r.cycles > 0 and r.realtime > 0
        assert r.bad_words == 0 and r.first_bad_offset == nodeagent.NO_BAD_OFFSET
        assert r.bad_phase == 0xFFFFFFFF and r.xor_mask == 0
        zero = (6, 7) if i < 9 else (0, 1, 2, 3, 4, 5, 7)
        assert all(r.checksum[p] == 0 for p in zero)
        assert all(r.checksum[p] != 0 for p in range(8) if p not in zero)


@pytest.mark.gpu
def test_gpu_xread_crosses_xcds(agent):
    """Of the second launch's workgroups, some read a slice another XCD wrote."""
    n = 9
    recs = _run(agent, n, 65536, 1)
    crossed = sum(recs[n + w].xcc != recs[(w + 1) % n].xcc for w in range(n))
    print(f"xread: {crossed} of {n} workgroups read a slice written on another XCC; readers "
          f"{[recs[n + w].xcc for w in range(n)]}, writers {[recs[w].xcc for w in range(n)]}")
    assert crossed > 0


@pytest.mark.gpu
def test_gpu_localisation_on_own_records(agent):
    n, slice_bytes = 9, 65536
    src = _run(agent, n, slice_bytes, 1)
    rc, res = agent.cache_sweep_verify(src, slice_bytes, 1)
    assert rc == nodeagent.NA_OK and res.ok and res.workgroups == n, agent._err()
    assert 0 < res.min_bytes_per_clk <= res.median_bytes_per_clk <= res.max_bytes_per_clk
    recs = (nodeagent.LdsRecord * len(src))()
    ctypes.memmove(recs, src, ctypes.sizeof(src))  # the shared run stays as it came back
    recs[4].checksum[2] ^= 1 << 17
    rc, res = agent.cache_sweep_verify(recs, slice_bytes, 1)
    assert rc == nodeagent.NA_ERR_VERIFY
    unit = (recs[4].xcc, recs[4].se, recs[4].sh, recs[4].cu)
    assert (res.bad_workgroups, res.bad_units, res.first_bad_workgroup) == (1, 1, 4)
    assert res.bad_cus == [unit] and res.first_bad_phase == "wt"
    assert nodeagent.mfma_unit_name(unit) in agent._err() and "phase wt" in agent._err()
    # the second launch's record, and who wrote what it read
    ctypes.memmove(recs, src, ctypes.sizeof(src))
    recs[n + 8].checksum[6] ^= 1
    rc, res = agent.cache_sweep_verify(recs, slice_bytes, 1)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.first_bad_workgroup, res.first_bad_phase) == (8, "xread")
    writer = (src[0].xcc, src[0].se, src[0].sh, src[0].cu)
    assert f"written by workgroup 0 on {nodeagent.mfma_unit_name(writer)}" in agent._err()


@pytest.mark.gpu
def test_gpu_default_sweep(agent):
    res = _default_sweep(agent)
    _, _, _, cus = agent.device_info(0)
    print(f"cache_sweep: {res.gbs:.1f} GB/s, per CU median {res.median_bytes_per_clk:.2f} min "
          f"{res.min_bytes_per_clk:.2f} max {res.max_bytes_per_clk:.2f} B/clk, "
          f"{res.clock_mhz:.0f} MHz, {res.units_seen} of {cus} CUs, {res.workgroups} workgroups")
    assert res.ok, res.describe()
    assert res.workgroups == 4 * cus and res.bad_workgroups == 0 and res.bad_cus == []
    assert res.units_seen == cus
    assert res.gbs > nodeagent.MIN_CACHE_SWEEP_GBS > 0
    # no documented per-CU ceiling for one latency-bound workgroup per CU: order only
    assert 0 < res.min_bytes_per_clk <= res.median_bytes_per_clk <= res.max_bytes_per_clk


@pytest.mark.gpu
def test_gpu_check_with_sweep(agent):
    torch.cuda.synchronize()
    report = agent.check(bw_bytes=1 << 28, cache_sweep=True)
    g0 = report.gpus[0]
    assert g0.healthy, g0.problems
    assert g0.cache_sweep_gbs > nodeagent.MIN_CACHE_SWEEP_GBS
    assert g0.cache_sweep_min_cu_bytes_per_clk > 0
    assert g0.cache_sweep_units_seen == g0.cus and g0.cache_sweep_bad_workgroups == 0


@pytest.mark.gpu
def test_gpu_cli_cache_sweep():
    _ensure_lib()
    proc = subprocess.run(
        [sys.executable, "-m", "gpu_provisioner_amd.nodeagent", "--json",
         "--bw-bytes", "268435456", "--cache-sweep"],
        capture_output=True,
        text=True,
        cwd=ROOT,
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    report = json.loads(proc.stdout)
    assert report["healthy"] is True
    g0 = report["gpus"][0]
    assert g0["cache_sweep_bad_workgroups"] == 0 and g0["cache_sweep_gbs"] > 0
    assert g0["cache_sweep_units_seen"] == g0["cus"]
