"""Chip-wide vector-unit sweep of the node agent (nodeagent/valusweep.h).

The reference for every exact checksum is the numpy simulation below, written
from the specification in the header: it keeps the 64 lanes of a wave as
vectors, fills and reads back the 480 register slots one by one, walks the
chains step by step in floating point where the phase is floating point
(float32, float64 and float16 arrays, so an inexact step would show), and
moves data between lanes with its own permutation tables. It shares nothing
with the host code, and known answers pin both. The transcendental phase has
no reference: it is checked by consensus among the records.

CPU: exported symbols, the host reference against numpy, the cross-lane
tables, the verify (attribution to SIMD and phase, the consensus phase, wave
index and placement), argument errors, check()/report/CLI/chart/docs behaviour
against a Python stand-in for the native library, and the kernel's register
budget from the compiler's remarks.
GPU (@pytest.mark.gpu, device 0): record checksums at the smallest shapes that
can go wrong, seed dependence, record sanity, localisation on the GPU's own
records (only HOST data is corrupted; nothing on the GPU is provoked), the
default sweep once, and the end-to-end CLI path.
"""
import ctypes
import functools
import json
import os
import re
import shutil
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEED = nodeagent.DEFAULT_VALU_SWEEP_SEED
PHASES = nodeagent.VALU_SWEEP_PHASES
EXACT = [p for p in range(9) if PHASES[p] != "trans"]
TRANS = PHASES.index("trans")
U64, U32 = np.uint64, np.uint32
LANE = np.arange(64)


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


def _h(seed, p, i):
    """h(p, i) for an array of indices."""
    with np.errstate(over="ignore"):
        return _mix64(U64((seed * G) & M64) + U64(p << 32) + np.asarray(i, dtype=U64))


def _fold(c, v):
    with np.errstate(over="ignore"):
        return c * U64(G) + v.astype(U64)


def _fold_int(c, v):
    """Signed values, sign-extended to 64 bits."""
    return _fold(c, np.asarray(v).astype(np.int64).view(U64))


def _total(c):
    return int(c.sum(dtype=U64))


def _ref_rf(seed, p, gl):
    pol = U32(0xFFFFFFFF if p else 0)
    regs = np.zeros((480, 64), dtype=U32)  # slot s: a0..a255, then v32..v255
    with np.errstate(over="ignore"):
        x = (_h(seed, p, gl) >> U64(32)).astype(U32)
        for s in range(480):
            x = x * U32(1664525) + U32(1013904223)
            regs[s] = x ^ pol
        assert len({int(v) for v in regs[:, 0]}) == 480  # no two slots of a lane alike
        lo = np.zeros(64, dtype=U32)
        hi = np.zeros(64, dtype=U32)
        for s in range(480):
            lo = lo * U32(0x9E3779B1) + regs[s]
            hi = hi * U32(0x85EBCA77) + regs[s]
    return _total((hi.astype(U64) << U64(32)) | lo.astype(U64))


def _ref_i32(seed, gl):
    h0, h1 = _h(seed, 2, 2 * gl), _h(seed, 2, 2 * gl + 1)
    lo32 = U64(0xFFFFFFFF)
    a, b, c, d = h0 & lo32, h0 >> U64(32), h1 & lo32, h1 >> U64(32)  # 32-bit values in uint64
    acc = np.zeros(64, dtype=U64)
    with np.errstate(over="ignore"):
        for k in range(64):
            t = (a * b) & lo32
            u = (c * (d | U64(1))) >> U64(32)
            m = a * c + ((d << U64(32)) | b)
            e = (t + u + (m & lo32)) & lo32
            f = e ^ (m >> U64(32)) ^ U64(k)
            g = (((f << U64(32)) | e) >> U64(k & 31)) & lo32
            gb = [(g >> U64(8 * i)) & U64(0xFF) for i in range(4)]
            tb = [(t >> U64(8 * i)) & U64(0xFF) for i in range(4)]
            q = gb[0] | (tb[3] << U64(8)) | (gb[2] << U64(16)) | (tb[1] << U64(24))
            acc = _fold(acc, (q << U64(32)) | g)
            acc = _fold(acc, (f << U64(32)) | e)
            a, b, c, d = (q + U64(0x9E3779B9)) & lo32, g | U64(1), f, (e + U64(k)) & lo32
    return _total(acc)


def _chain_params(seed, p, first, n, mask):
    """x, a, b of chains first..first+n-1 of every lane: arrays [n][64] of ints."""
    e = np.stack([_h(seed, p, first + j) for j in range(n)])
    x = (e & U64(mask)).astype(np.int64) - (mask + 1) // 2
    a = ((e >> U64(12)) % U64(7)).astype(np.int64) - 3
    b = ((e >> U64(20)) % U64(15)).astype(np.int64) - 7
    return x, a, b


def _fma(x, a, b, dtype):
    """One fused multiply-add per element in `dtype`: the product is formed
    exactly (in float64, or for float64 in Python integers) and rounded once."""
    if dtype == np.float64:
        exact = x.astype(np.int64) * a.astype(np.int64) + b.astype(np.int64)
        assert np.all(x == x.astype(np.int64)) and np.all(np.abs(exact) < 2 ** 53)
        return exact.astype(np.float64)
    wide = x.astype(np.float64) * a.astype(np.float64) + b.astype(np.float64)
    out = wide.astype(dtype)
    assert np.all(out.astype(np.float64) == wide)  # the spec's claim: every step is exact
    return out


def _ref_chains(seed, p, gl, groups, steps=64):
    """groups: (chains, mask, dtype) in chain order; a step runs all chains
    in order, each through fma -> int -> fold -> re-centre -> back."""
    state, first = [], 0
    for n, mask, dtype in groups:
        x, a, b = _chain_params(seed, p, sum(g[0] for g in groups) * gl + first, n, mask)
        state.append([x.astype(dtype), a.astype(dtype), b.astype(dtype), mask, dtype])
        first += n
    acc = np.zeros(64, dtype=U64)
    for _ in range(steps):
        for st in state:
            x, a, b, mask, dtype = st
            for j in range(len(x)):
                r = _fma(x[j], a[j], b[j], dtype).astype(np.int32)
                acc = _fold_int(acc, r)
                x[j] = ((r & np.int32(mask)) - np.int32((mask + 1) // 2)).astype(dtype)
    return _total(acc)


# -- cross-lane moves, from the ISA's description of each --------------------


def _swap_table(half):
    """v_permlane{16,32}_swap on the 128 slots A[0..63], B[0..63]: the odd
    rows (of `half` lanes) of A trade places with the even rows of B."""
    src = np.arange(128)
    for lane in range(64):
        if lane & half:  # A's odd row <- B's even row below it, and back
            src[lane] = 64 + lane - half
            src[64 + lane - half] = lane
    return src


XLANE_TABLES = [
    (LANE & ~3) | np.array([1, 2, 3, 0])[LANE & 3],  # quad_perm:[1,2,3,0]
    (LANE & ~15) | ((LANE - 3) & 15),                # row_ror:3: data moves 3 lanes up, wrapping
    (LANE & ~15) | (15 - (LANE & 15)),               # row_mirror
    (LANE & ~7) | (7 - (LANE & 7)),                  # row_half_mirror
    (5 * LANE + 3) & 63,                             # ds_bpermute: lane reads lane index
    _swap_table(16),
    _swap_table(32),
    np.full(64, 37),                                 # v_readlane broadcast
]


def _ref_xlane(seed, gl):
    v = (_h(seed, 6, gl) >> U64(32)).astype(U32)
    acc = np.zeros(64, dtype=U64)
    with np.errstate(over="ignore"):
        for n, table in enumerate(XLANE_TABLES):
            if len(table) == 128:
                both = np.concatenate([v, v ^ U32(0xA5A5A5A5 if n == 5 else 0x5A5A5A5A)])[table]
                a, b = both[:64], both[64:]
                moved = a ^ ((b << U32(7)) | (b >> U32(25)))
            else:
                moved = v[table]
            v = moved * U32(0x9E3779B1) + LANE.astype(U32)
            acc = _fold(acc, v)
    return _total(acc)


def _ref_stream(seed, gl, iters):
    """The rounds themselves, in float32, not the closed form."""
    e = np.stack([_h(seed, 8, 32 * gl + j) for j in range(32)])
    x = ((e & U64(0xFFF)).astype(np.int64) - 2048).astype(np.float32)
    s = np.where((e >> U64(12)) & U64(1), -1.0, 1.0).astype(np.float32)
    b = (((e >> U64(13)) % U64(5)).astype(np.int64) - 2).astype(np.float32)
    for _ in range(iters):
        x = _fma(x, s, b, np.float32)
    acc = np.zeros(64, dtype=U64)
    for j in range(32):
        acc = _fold_int(acc, x[j].astype(np.int32))
    return _total(acc)


@functools.lru_cache(maxsize=None)
def _ref_fixed(seed, wave):
    """The phases that do not depend on iters."""
    gl = (wave * 64 + LANE).astype(U64)
    return (
        _ref_rf(seed, 0, gl), _ref_rf(seed, 1, gl), _ref_i32(seed, gl),
        _ref_chains(seed, 3, gl, [(4, 0xFFF, np.float32)]),
        _ref_chains(seed, 4, gl, [(4, 0xFFF, np.float64)]),
        _ref_chains(seed, 5, gl, [(4, 0xFFF, np.float32), (4, 0x3FF, np.float16)]),
        _ref_xlane(seed, gl),
    )


@functools.lru_cache(maxsize=None)
def ref_checksums(seed, wave, iters):
    """The nine phase checksums of one wave, in the order of PHASES; trans 0."""
    gl = (wave * 64 + LANE).astype(U64)
    return list(_ref_fixed(seed, wave)) + [0, _ref_stream(seed, gl, iters)]


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------

SYMBOLS = ("na_valu_sweep_slots", "na_valu_sweep_expected", "na_valu_sweep_run",
           "na_valu_sweep_verify", "na_valu_sweep", "na_valu_sweep_xlane_table")


def test_library_exports_valu_sweep_symbols():
    lib = ctypes.CDLL(_ensure_lib())
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing symbol {sym}"


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


def test_constants(cpu_agent):
    assert SEED.to_bytes(8, "big") == b"MI355XVS"
    assert PHASES == ("rf", "rf_inv", "i32", "f32", "f64", "pk", "xlane", "trans", "stream")
    assert ctypes.sizeof(nodeagent.ValuRecord) == 128
    # R = 512 - F with F <= 64: at least 448 of the 512 registers per lane
    assert cpu_agent.valu_sweep_slots() == 512 - nodeagent.VALU_SWEEP_FIRST_VGPR == 480
    assert nodeagent.VALU_SWEEP_FIRST_VGPR <= 64
    assert nodeagent.VALU_SWEEP_PEAK_FLOP_PER_CLK == 64
    # the stream phase stays exact: |x0| + 2 iters < 2^24
    assert 2048 + 2 * nodeagent.VALU_SWEEP_MAX_ITERS < 1 << 24
    assert 2048 + 2 * (nodeagent.VALU_SWEEP_MAX_ITERS + 2) >= 1 << 24
    assert nodeagent.valu_slot_name(0) == "a0" and nodeagent.valu_slot_name(255) == "a255"
    assert nodeagent.valu_slot_name(256) == "v32" and nodeagent.valu_slot_name(479) == "v255"
    assert nodeagent.valu_slot_name(512 + 300) == "v76"


KNOWN = (SEED, 5, 7, [
    "0x3a099b9f3efbae40", "0x12e72c5f0ea4c8e0", "0x960db4c6aa3e559c", "0xdcd3a0f77c1ed5a0",
    "0x4e82cd94234485ce", "0xc312ec86c2b1effa", "0x10f00185f3e4507b", "0x0000000000000000",
    "0x8ab18dc0f74cd909"])


def test_reference_known_answers(cpu_agent):
    seed, wave, iters, want = KNOWN
    got = ref_checksums(seed, wave, iters)
    assert [f"{x:#018x}" for x in got] == want
    assert cpu_agent.valu_sweep_expected(wave, iters, seed) == got


@pytest.mark.parametrize("seed", [7, SEED])
@pytest.mark.parametrize("wave", [0, 1, 5, 1023])
def test_expected_checksums_match_reference(cpu_agent, seed, wave):
    for iters in (1, 2, 7):
        want = ref_checksums(seed, wave, iters)
        got = cpu_agent.valu_sweep_expected(wave, iters, seed)
        assert got[TRANS] == 0
        assert got == want, (iters, [PHASES[p] for p in range(9) if got[p] != want[p]])


def test_stream_closed_form_at_the_exactness_bound(cpu_agent):
    """The host's closed form at iters the simulation cannot walk: every chain
    ends within the integers float32 holds exactly."""
    top = nodeagent.VALU_SWEEP_MAX_ITERS
    gl = (3 * 64 + LANE).astype(U64)
    e = np.stack([_h(SEED, 8, 32 * gl + j) for j in range(32)])
    x = (e & U64(0xFFF)).astype(np.int64) - 2048
    neg = ((e >> U64(12)) & U64(1)).astype(bool)
    b = ((e >> U64(13)) % U64(5)).astype(np.int64) - 2
    for iters in (top, top - 1):
        end = np.where(neg, b - x if iters & 1 else x, x + iters * b)
        assert np.abs(end).max() < 1 << 24
        acc = np.zeros(64, dtype=U64)
        for j in range(32):
            acc = _fold_int(acc, end[j])
        assert cpu_agent.valu_sweep_expected(3, iters)[8] == _total(acc)


def test_reference_depends_on_seed_wave_and_iters():
    a = ref_checksums(SEED, 1, 2)
    for other in (ref_checksums(SEED + 1, 1, 2), ref_checksums(SEED, 2, 2)):
        assert all(a[p] != other[p] for p in EXACT)
    c = ref_checksums(SEED, 1, 3)
    assert a[:8] == c[:8] and a[8] != c[8]


def test_xlane_tables(cpu_agent):
    """Host and simulation agree on every move; all but the broadcast are
    bijections, and the two swaps are involutions."""
    assert len(XLANE_TABLES) == nodeagent.VALU_SWEEP_XLANE_MOVES
    for n, table in enumerate(XLANE_TABLES):
        host = cpu_agent.valu_sweep_xlane_table(n)
        assert host == [int(x) for x in table], n
        if n == 7:
            assert set(host) == {37}
            continue
        assert sorted(host) == list(range(len(host))), n
        # no move is the identity, and the DPP ones stay inside their row
        assert any(s != i for i, s in enumerate(host))
        if n < 4:
            assert all(s // 16 == i // 16 for i, s in enumerate(host))
    for n, half in ((5, 16), (6, 32)):
        t = np.array(cpu_agent.valu_sweep_xlane_table(n))
        assert np.array_equal(t[t], np.arange(128))
        # e.g. permlane32_swap: lanes 32..63 of A <-> lanes 0..31 of B, rest in place
        moved = [i for i in range(128) if t[i] != i]
        assert moved == [i for i in range(64) if i & half] + \
            [64 + i for i in range(64) if not i & half]
    assert list(XLANE_TABLES[6][32:64]) == list(range(64, 96))
    lib = cpu_agent.lib
    out = (ctypes.c_int * 128)()
    for move, ptr, n in [(-1, out, 128), (8, out, 128), (0, None, 128), (0, out, 63), (5, out, 64)]:
        assert lib.na_valu_sweep_xlane_table(move, ptr, n) == nodeagent.NA_ERR_ARG
        assert "na_valu_sweep_xlane_table" in cpu_agent._err()


def _unit_of(wave):
    """A made-up placement: workgroup g on CU g, its waves on SIMDs 3, 2, 1, 0."""
    g = wave // 4
    return (g % 8, (g // 8) % 4, (g // 32) % 2, (g // 64) % 16, 3 - wave % 4)


ITERS = 2
CONSENSUS = 0x1234_5678_9ABC_DEF0


def _records(n, iters=ITERS, seed=SEED):
    recs = (nodeagent.ValuRecord * n)()
    for i in range(n):
        r = recs[i]
        r.checksum[:] = ref_checksums(seed, i, iters)
        r.checksum[TRANS] = CONSENSUS
        # 40, 41, ... FLOP per clock
        r.cycles, r.realtime, r.wave = iters * 4096 * 1000 // (40 + i), 40, i
        r.xcc, r.se, r.sh, r.cu, r.simd = _unit_of(i)
        r.rf_bad, r.rf_first_slot, r.rf_first_lane, r.rf_xor = 0, 0xFFFFFFFF, 0xFFFFFFFF, 0
    return recs


def test_verify_clean_records(cpu_agent):
    recs = _records(12)
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_OK and res.ok, cpu_agent._err()
    assert (res.waves, res.bad_waves, res.cus_seen, res.simds_seen) == (12, 0, 3, 12)
    assert res.bad == [] and not res.trans_unchecked and res.trans_consensus == CONSENSUS
    assert res.rf_bad == 0 and res.rf_first_slot == nodeagent.NO_BAD_SLOT
    # the same records do not verify under other rounds or another seed
    bad = cpu_agent.valu_sweep_verify(recs, 3)[1]
    assert bad.bad_waves == 12 and bad.bad[0][2] == ["stream"]
    bad = cpu_agent.valu_sweep_verify(recs, ITERS, SEED + 1)[1]
    assert bad.bad_waves == 12 and bad.bad[0][2] == [PHASES[p] for p in EXACT]


def test_verify_rate_statistics(cpu_agent):
    recs = _records(12)
    rates = sorted(ITERS * 4096 / recs[i].cycles for i in range(12))
    _, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert res.median_flop_per_clk == pytest.approx(rates[6], rel=1e-12)
    assert res.min_flop_per_clk == pytest.approx(rates[0], rel=1e-12)
    cycles = sorted(recs[i].cycles for i in range(12))
    assert res.median_cycles == cycles[6]
    mhz = sorted(recs[i].cycles / 40 * 100.0 for i in range(12))
    assert res.clock_mhz == pytest.approx(mhz[6], rel=1e-12)
    # from the in-kernel stamps alone: median SIMD rate x SIMDs seen x clock
    assert res.tflops == pytest.approx(rates[6] * 12 * mhz[6] / 1e6, rel=1e-12)


@pytest.mark.parametrize("phase", EXACT)
def test_verify_one_flipped_bit_names_unit_and_phase(cpu_agent, phase):
    recs = _records(12)
    wave = 1 + phase
    recs[wave].checksum[phase] ^= 1 << (phase * 7)
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
    assert res.bad_waves == 1 and res.bad == [(wave, _unit_of(wave), [PHASES[phase]])]
    name = nodeagent.mfma_unit_name(_unit_of(wave))
    assert f"1 of 12 waves wrong, first wave {wave} in phase {PHASES[phase]} on {name}" in \
        cpu_agent._err()
    assert name in res.describe() and f"({PHASES[phase]})" in res.describe()
    assert ".simd" in name


def test_verify_two_phases_of_one_wave(cpu_agent):
    recs = _records(8)
    recs[6].checksum[4] ^= 1
    recs[6].checksum[6] ^= 1 << 63
    _, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert res.bad == [(6, _unit_of(6), ["f64", "xlane"])]
    assert "in phase f64,xlane on" in cpu_agent._err()


def test_verify_trans_minority_is_flagged(cpu_agent):
    recs = _records(12)
    recs[9].checksum[TRANS] ^= 1 << 20
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert res.bad == [(9, _unit_of(9), ["trans"])] and not res.trans_unchecked
    assert res.trans_consensus == CONSENSUS
    # three records, two alike: the odd one out, wherever it sits
    for odd in range(3):
        recs = _records(3)
        recs[odd].checksum[TRANS] = 99
        _, res = cpu_agent.valu_sweep_verify(recs, ITERS)
        assert [b[0] for b in res.bad] == [odd] and res.bad[0][2] == ["trans"]


def test_verify_trans_unchecked_is_not_a_failure(cpu_agent):
    # two records cannot outvote each other
    recs = _records(2)
    recs[1].checksum[TRANS] ^= 1
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_OK and res.ok and res.trans_unchecked and res.trans_consensus == 0
    # no strict majority: 2 of 4, and three different values
    recs = _records(4)
    recs[0].checksum[TRANS] = recs[1].checksum[TRANS] = 5
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_OK and res.trans_unchecked
    recs = _records(3)
    recs[0].checksum[TRANS], recs[1].checksum[TRANS] = 5, 6
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_OK and res.trans_unchecked
    # an exact phase still fails such a set
    recs[2].checksum[0] ^= 1
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY and res.trans_unchecked and res.bad[0][2] == ["rf"]


def test_verify_duplicated_and_missing_wave(cpu_agent):
    recs = _records(12)
    recs[5].wave = 4  # wave 4 twice, wave 5 never
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert res.bad == [(5, _unit_of(5), ["index"])]
    assert "first wave 5 in phase index" in cpu_agent._err()
    # a wave that never wrote its record
    recs = _records(12)
    ctypes.memset(ctypes.byref(recs[7]), 0xFF, ctypes.sizeof(nodeagent.ValuRecord))
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY and res.bad_waves == 4  # and its workgroup's placement
    assert "index" in dict((b[0], b[2]) for b in res.bad)[7]


def test_verify_unwritten_records_median_cycles_is_the_integer_itself(cpu_agent):
    """Eight records no wave wrote: every cycle count is 2^64 - 1, which a
    median taken through double would round to 2^64 and convert back out of
    range."""
    recs = (nodeagent.ValuRecord * 8)()
    ctypes.memset(recs, 0xFF, ctypes.sizeof(recs))
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert res.median_cycles == 2**64 - 1
    assert res.bad_waves == 8


def test_verify_workgroup_not_on_four_simds_of_one_cu(cpu_agent):
    recs = _records(12)
    recs[6].simd = recs[5].simd  # two waves of workgroup 1 on one SIMD
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert [(b[0], b[2]) for b in res.bad] == [(w, ["placement"]) for w in (4, 5, 6, 7)]
    recs = _records(12)
    recs[9].cu += 1  # four SIMDs, two CUs
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert [(b[0], b[2]) for b in res.bad] == [(w, ["placement"]) for w in (8, 9, 10, 11)]
    assert "in phase placement on" in cpu_agent._err()


def test_verify_in_kernel_diagnosis_with_correct_checksums_is_bad(cpu_agent):
    recs = _records(8)
    r = recs[3]
    r.rf_bad, r.rf_first_slot, r.rf_first_lane, r.rf_xor = 3, 512 + 300, 41, 0x00000100
    rc, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY and res.bad == [(3, _unit_of(3), ["rf_inv"])]
    assert (res.rf_bad, res.rf_first_slot, res.rf_first_lane, res.rf_xor) == (3, 812, 41, 0x100)
    assert "3 wrong registers, first v76 lane 41, failing bits 0x00000100" in cpu_agent._err()
    assert "first v76 inverted lane 41, failing bits 0x00000100" in res.describe()
    r.rf_first_slot = 17
    _, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert res.bad[0][2] == ["rf"] and "first a17 lane 41" in res.describe()


def test_verify_lists_at_most_eight_waves_and_keeps_the_count(cpu_agent):
    recs = _records(12)
    for i in range(12):
        recs[i].checksum[2] ^= 1
    _, res = cpu_agent.valu_sweep_verify(recs, ITERS)
    assert res.bad_waves == 12 and len(res.bad) == nodeagent.VALU_SWEEP_MAX_LISTED == 8
    assert [b[0] for b in res.bad] == list(range(8))
    assert "12 of 12 waves wrong" in res.describe() and ", ..." in res.describe()


def test_argument_errors_before_any_hip_call(cpu_agent):
    lib = cpu_agent.lib
    recs = (nodeagent.ValuRecord * 8)()
    out = (ctypes.c_uint64 * 9)()
    ms = ctypes.c_double(0)
    seed, i64, u64 = ctypes.c_ulonglong(SEED), ctypes.c_longlong, ctypes.c_ulonglong
    res = nodeagent._ValuSweepResultC()
    top = nodeagent.VALU_SWEEP_MAX_ITERS

    for iters, ptr in [(0, out), (-1, out), (top + 1, out), (1, None)]:
        assert lib.na_valu_sweep_expected(seed, u64(0), iters, ptr) == nodeagent.NA_ERR_ARG
        assert "na_valu_sweep_expected" in cpu_agent._err()
    assert lib.na_valu_sweep_expected(seed, u64(0), top, out) == nodeagent.NA_OK

    def run(workgroups, iters, out_, n_out):
        return lib.na_valu_sweep_run(0, workgroups, iters, seed, out_, i64(n_out), ctypes.byref(ms))

    for args in [(0, 1, recs, 8), (-2, 1, recs, 8), ((1 << 20) + 1, 1, recs, 8), (2, 0, recs, 8),
                 (2, -1, recs, 8), (2, top + 1, recs, 8), (2, 1, None, 8), (2, 1, recs, 7)]:
        assert run(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_valu_sweep_run" in cpu_agent._err()

    def verify(r, n, iters, out_):
        return lib.na_valu_sweep_verify(r, i64(n), iters, seed, out_)

    for args in [(None, 8, 1, ctypes.byref(res)), (recs, 0, 1, ctypes.byref(res)),
                 (recs, 8, 0, ctypes.byref(res)), (recs, 8, top + 1, ctypes.byref(res)),
                 (recs, 8, 1, None)]:
        assert verify(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_valu_sweep_verify" in cpu_agent._err()

    for args in [(-1, 0, ctypes.byref(res)), ((1 << 20) + 1, 0, ctypes.byref(res)),
                 (0, -1, ctypes.byref(res)), (0, top + 1, ctypes.byref(res)), (0, 0, None)]:
        assert lib.na_valu_sweep(0, args[0], args[1], seed, args[2]) == nodeagent.NA_ERR_ARG, args
        assert "na_valu_sweep:" in cpu_agent._err()
    with pytest.raises(nodeagent.NodeAgentError):
        cpu_agent.valu_sweep_run(0, workgroups=0)
    with pytest.raises(nodeagent.NodeAgentError):
        cpu_agent.valu_sweep_expected(0, top + 1)


# -- check() against a Python stand-in library --------------------------------

SICK_SIMD = (5, 2, 1, 9, 3)


class FakeLib(LdsFakeLib):
    """The LDS sweep's stand-in plus na_valu_sweep. ``valu``: {dev: "sick" |
    "slow" | "fewer" | "unchecked"}; default clean. A sick GPU has one SIMD
    whose four waves all fail the f64 phase."""

    def __init__(self, ngpu=1, valu=None):
        super().__init__(ngpu=ngpu)
        self.valu_calls = []
        valu = valu or {}

        def na_valu_sweep(dev, workgroups, iters, seed, res):
            self.valu_calls.append((dev, workgroups, iters, seed.value))
            kind = valu.get(dev, "ok")
            r = res._obj
            r.waves, r.cus_seen, r.clock_mhz = 4096, 256, 2391.7
            r.simds_seen = 1023 if kind == "fewer" else 1024
            r.trans_unchecked, r.trans_consensus = int(kind == "unchecked"), 0xABCD
            r.bad_waves, r.listed, r.rf_bad = 0, 0, 0
            r.median_flop_per_clk, r.min_flop_per_clk = 63.2, 61.456
            r.tflops = 0.12 if kind == "slow" else 154.76
            if kind != "sick":
                return 0
            r.bad_waves, r.listed = 4, 4
            for k in range(4):
                r.bad_list[k][:] = (403 + 1024 * k,) + SICK_SIMD + (1 << 4,)
            return nodeagent.NA_ERR_VERIFY

        self.na_valu_sweep = na_valu_sweep


def _agent(monkeypatch, **kw):
    fake = FakeLib(**kw)
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fake)
    return nodeagent.NodeAgent(), fake


def _sweep_fields(g):
    return (g.valu_sweep_tflops, g.valu_sweep_min_simd_flop_per_clk, g.valu_sweep_simds_seen,
            g.valu_sweep_bad_waves, g.valu_sweep_trans_unchecked)


def test_check_default_never_runs_sweep(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check()
    assert fake.valu_calls == [] and fake.lds_calls == [] and fake.sweep_calls == []
    assert report.healthy, report.problems
    assert _sweep_fields(report.gpus[0]) == (0.0, 0.0, 0, 0, False)
    assert _sweep_fields(nodeagent.GPUReport(index=0)) == (0.0, 0.0, 0, 0, False)
    # the stand-in of the LDS sweep's tests has no vector-unit sweep at all
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: LdsFakeLib())
    monkeypatch.setattr(nodeagent, "MIN_LDS_SWEEP_GBS", 80000.0)
    assert nodeagent.NodeAgent().check(lds_sweep=True).healthy


def test_check_clean_sweep_populates_fields(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_VALU_SWEEP_TFLOPS", 100.0)
    agent, fake = _agent(monkeypatch)
    report = agent.check(valu_sweep=True)
    assert fake.valu_calls == [(0, 0, 0, SEED)] and fake.lds_calls == []
    g = report.gpus[0]
    assert report.healthy and g.healthy, report.problems
    assert _sweep_fields(g) == (154.8, 61.46, 1024, 0, False)
    assert nodeagent.node_condition_from_report(report)["status"] == "True"
    assert json.loads(json.dumps(nodeagent.asdict(report)))["gpus"][0]["valu_sweep_tflops"] == 154.8


def test_check_fewer_simds_and_unchecked_trans_are_reported_not_problems(monkeypatch):
    agent, _ = _agent(monkeypatch, valu={0: "fewer"})
    report = agent.check(valu_sweep=True)
    assert report.gpus[0].valu_sweep_simds_seen == 1023 < 4 * report.gpus[0].cus
    assert report.healthy, report.problems
    agent, _ = _agent(monkeypatch, valu={0: "unchecked"})
    report = agent.check(valu_sweep=True)
    assert report.gpus[0].valu_sweep_trans_unchecked is True and report.healthy


def test_check_eight_gpus_one_sick_simd(monkeypatch):
    agent, fake = _agent(monkeypatch, ngpu=8, valu={3: "sick"})
    report = agent.check(expect_gpus=8, valu_sweep=True)
    assert [c[0] for c in fake.valu_calls] == list(range(8))
    unit = "xcc5.se2.sh1.cu9.simd3 (f64)"
    assert report.problems == [f"gpu3: VALU sweep: 4 of 4096 waves wrong: {', '.join([unit] * 4)}"]
    assert not report.healthy
    assert [g.healthy for g in report.gpus] == [i != 3 for i in range(8)]
    assert [g.valu_sweep_bad_waves for g in report.gpus] == [4 * (i == 3) for i in range(8)]
    cond = nodeagent.node_condition_from_report(report)
    assert cond["status"] == "False" and "xcc5.se2.sh1.cu9.simd3" in cond["message"]


def test_check_low_rate_flags_a_problem(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_VALU_SWEEP_TFLOPS", 100.0)
    agent, _ = _agent(monkeypatch, valu={0: "slow"})
    report = agent.check(valu_sweep=True)
    assert report.gpus[0].problems == ["VALU sweep 0.1 TFLOP/s below floor 100.0"]
    assert not report.healthy
    assert nodeagent.node_condition_from_report(report)["status"] == "False"


def _profile_lines(key):
    with open(os.path.join(ROOT, "profiles", "valu_sweep_mi355x.txt")) as f:
        return [line.split()[1:] for line in f if line.startswith(key + " ")]


def test_floor_is_derived_from_the_profile():
    """0.70 x the median of the profile's per-process figures, and below the
    ceiling of 64 FLOP per clock and SIMD."""
    runs = [float(x) for row in _profile_lines("tflops") for x in row]
    assert len(runs) >= 5
    assert nodeagent.MIN_VALU_SWEEP_TFLOPS == pytest.approx(0.70 * float(np.median(runs)), abs=0.06)
    assert 0 < nodeagent.MIN_VALU_SWEEP_TFLOPS < 157.3
    # "flop_per_clk_per_simd median|min" rows: the label, then the figures
    per_simd = [float(x) for row in _profile_lines("flop_per_clk_per_simd") for x in row[1:]]
    assert len(per_simd) >= 10 and all(0 < x <= nodeagent.VALU_SWEEP_PEAK_FLOP_PER_CLK for x in per_simd)


def test_cli_flag_reaches_check(monkeypatch, capsys):
    _, fake = _agent(monkeypatch)
    assert nodeagent.main(["--valu-sweep"]) == 0
    assert [c[0] for c in fake.valu_calls] == [0]
    assert json.loads(capsys.readouterr().out)["gpus"][0]["valu_sweep_simds_seen"] == 1024
    _, fake = _agent(monkeypatch)
    assert nodeagent.main([]) == 0
    assert fake.valu_calls == []
    capsys.readouterr()


def test_chart_passes_valu_sweep_only_when_true():
    import yaml

    chart = os.path.join(ROOT, "charts", "gpu-provisioner-amd")
    with open(os.path.join(chart, "values.yaml")) as f:
        values = yaml.safe_load(f)
    assert values["nodeAgent"]["valuSweep"] is False
    with open(os.path.join(chart, "templates", "amd-gpu-node-stack.yaml")) as f:
        text = f.read()
    start = text.index("{{- if .Values.nodeAgent.valuSweep }}")
    end = text.index("{{- end }}", start)
    assert "--valu-sweep \\" in text[start:end]
    assert text.count("--valu-sweep") == 1  # nowhere outside the guard


def test_docs_cover_the_sweep():
    with open(os.path.join(ROOT, "docs", "METRICS.md")) as f:
        metrics = f.read()
    for name in ("valu_sweep_tflops", "valu_sweep_min_simd_flop_per_clk", "valu_sweep_simds_seen",
                 "valu_sweep_bad_waves", "valu_sweep_trans_unchecked"):
        assert name in metrics, name
        assert hasattr(nodeagent.GPUReport(index=0), name)
    for doc in ("docs/DESIGN.md", "docs/OPERATIONS.md", "README.md"):
        with open(os.path.join(ROOT, doc)) as f:
            assert "--valu-sweep" in f.read(), doc
    with open(os.path.join(ROOT, "docs", "DESIGN.md")) as f:
        design = f.read()
    # what the sweep does not cover is said where it is described
    for gap in ("v0..v31", "SGPR", "conversion", "common to the whole chip", "thermal soak"):
        assert gap in design, gap


def test_kernel_register_budget_from_compiler_remarks(tmp_path):
    """The register-file phases name a0..a255 and v32..v255: the kernel must
    get all 512 registers, one wave per SIMD, and keep nothing in scratch.
    Reads the compiler's resource-usage remarks only."""
    hipcc = shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("hipcc not installed")
    src = tmp_path / "valusweep_audit.hip"
    src.write_text('#include "valusweep.h"\n')
    proc = subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "-c", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage", "-I", os.path.join(ROOT, "nodeagent"),
         str(src), "-o", str(tmp_path / "valusweep_audit.o")],
        capture_output=True, text=True,
    )
    assert proc.returncode == 0, proc.stderr
    remarks = proc.stderr
    at = remarks.index("valu_sweep_kernel")
    block = remarks[at:remarks.index("LDS Size", at)]
    # "...: remark:     VGPRs: 256 [-Rpass-analysis=...]", some keys with a unit in brackets
    found = {k: int(v)
             for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", block)}
    print(found)
    assert found["VGPRs"] == 256 and found["AGPRs"] == 256
    assert found["ScratchSize"] == 0 and found["VGPRs Spill"] == 0
    assert found["Occupancy"] == 1


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


_runs = {}


def _run(agent, workgroups, iters, seed=SEED):
    """One launch per distinct shape, shared by the tests; read-only."""
    key = (workgroups, iters, seed)
    if key not in _runs:
        torch.cuda.synchronize()
        _runs[key] = agent.valu_sweep_run(0, workgroups, iters, seed)[0]
    return _runs[key]


_sweeps = []


def _default_sweep(agent):
    if not _sweeps:
        torch.cuda.synchronize()
        _sweeps.append(agent.valu_sweep(0))
    return _sweeps[0]


# 1 x 1: one workgroup, one stream round (an odd count: the s = -1 chains end
# at b - x); 2 x 3: a second workgroup's wave indices, several rounds
@pytest.mark.gpu
@pytest.mark.parametrize("workgroups,iters", [(1, 1), (2, 3)])
def test_gpu_record_checksums_match_reference(agent, workgroups, iters):
    recs = _run(agent, workgroups, iters)
    assert len(recs) == 4 * workgroups
    for w, r in enumerate(recs):
        want = ref_checksums(SEED, w, iters)
        got = list(r.checksum)
        print(f"wave {w}:", [f"{x:#x}" for x in got], r.rf_bad, r.rf_first_slot, r.rf_first_lane,
              hex(r.rf_xor))
        assert [got[p] for p in EXACT] == [want[p] for p in EXACT], \
            [PHASES[p] for p in EXACT if got[p] != want[p]]
        assert (r.rf_bad, r.rf_first_slot, r.rf_first_lane, r.rf_xor) == \
            (0, nodeagent.NO_BAD_SLOT, nodeagent.NO_BAD_SLOT, 0)
    assert len({r.checksum[TRANS] for r in recs}) == 1


@pytest.mark.gpu
def test_gpu_seed_changes_every_exact_phase_and_not_trans(agent):
    recs = _run(agent, 2, 3)
    other = _run(agent, 2, 3, seed=7)
    for w in range(8):
        assert all(recs[w].checksum[p] != other[w].checksum[p] for p in EXACT)
        assert recs[w].checksum[TRANS] == other[w].checksum[TRANS]
        want = ref_checksums(7, w, 3)
        assert [other[w].checksum[p] for p in EXACT] == [want[p] for p in EXACT]


@pytest.mark.gpu
def test_gpu_record_sanity(agent):
    recs = _run(agent, 2, 3)
    assert [r.wave for r in recs] == list(range(8))
    for g in range(2):
        group = recs[4 * g:4 * g + 4]
        assert len({(r.xcc, r.se, r.sh, r.cu) for r in group}) == 1
        assert sorted(r.simd for r in group) == [0, 1, 2, 3]
    for r in recs:
        assert r.xcc < 8 and r.se < 4 and r.sh < 2 and r.cu < 16
        assert r.cycles > 0 and r.realtime > 0


@pytest.mark.gpu
def test_gpu_localisation_on_own_records(agent):
    src = _run(agent, 2, 3)
    rc, res = agent.valu_sweep_verify(src, 3)
    assert rc == nodeagent.NA_OK and res.ok and res.waves == 8, agent._err()
    assert (res.cus_seen, res.simds_seen) == (len({(r.xcc, r.se, r.sh, r.cu) for r in src}), 8)
    assert not res.trans_unchecked and res.trans_consensus == src[0].checksum[TRANS]
    recs = (nodeagent.ValuRecord * len(src))()
    ctypes.memmove(recs, src, ctypes.sizeof(src))  # the shared run stays as it came back
    recs[5].checksum[4] ^= 1 << 17
    recs[2].checksum[TRANS] ^= 1
    rc, res = agent.valu_sweep_verify(recs, 3)
    assert rc == nodeagent.NA_ERR_VERIFY and res.bad_waves == 2
    units = [(r.xcc, r.se, r.sh, r.cu, r.simd) for r in recs]
    assert res.bad == [(2, units[2], ["trans"]), (5, units[5], ["f64"])]
    assert nodeagent.mfma_unit_name(units[2]) in agent._err() and "phase trans" in agent._err()
    assert nodeagent.mfma_unit_name(units[5]) in res.describe()


@pytest.mark.gpu
def test_gpu_default_sweep(agent):
    res = _default_sweep(agent)
    _, _, _, cus = agent.device_info(0)
    peak = nodeagent.VALU_SWEEP_PEAK_FLOP_PER_CLK
    ceiling = 4 * cus * peak * res.clock_mhz / 1e6
    print(f"valu_sweep: {res.tflops:.1f} TFLOP/s (ceiling {ceiling:.1f}), per SIMD median "
          f"{res.median_flop_per_clk:.2f} min {res.min_flop_per_clk:.2f} FLOP/clk, "
          f"{res.clock_mhz:.0f} MHz, {res.median_cycles} cycles, {res.simds_seen} SIMDs on "
          f"{res.cus_seen} of {cus} CUs, {res.waves} waves, trans {res.trans_consensus:#x}")
    assert res.ok, res.describe()
    assert res.waves == 16 * cus and res.bad_waves == 0 and res.bad == []
    assert res.cus_seen == cus and res.simds_seen == 4 * cus
    assert not res.trans_unchecked
    assert res.tflops >= nodeagent.MIN_VALU_SWEEP_TFLOPS > 0
    # the physical ceiling: a figure above it means the timing is wrong
    assert 0 < res.min_flop_per_clk <= res.median_flop_per_clk <= peak
    assert res.tflops <= ceiling


@pytest.mark.gpu
def test_gpu_cli_valu_sweep():
    _ensure_lib()
    proc = subprocess.run(
        [sys.executable, "-m", "gpu_provisioner_amd.nodeagent", "--json",
         "--bw-bytes", "268435456", "--valu-sweep"],
        capture_output=True,
        text=True,
        cwd=ROOT,
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    report = json.loads(proc.stdout)
    assert report["healthy"] is True
    g0 = report["gpus"][0]
    assert g0["valu_sweep_bad_waves"] == 0 and g0["valu_sweep_tflops"] > 0
    assert g0["valu_sweep_simds_seen"] == 4 * g0["cus"]
    assert g0["valu_sweep_trans_unchecked"] is False
