"""Chip-wide load sweep of the node agent (nodeagent/loadsweep.h): the
matrix-core sweep's MFMA chain on four waves of every CU while the other four
stream pattern-filled device memory through LDS and compare every word.

The reference for the stream checksums is the numpy simulation below, written
from the specification in the header: it builds the slice's memory image from
the memtest pattern, walks the four stream waves through their loads, their
LDS slots and the rotated read-back, and sums what each lane would get back.
It shares nothing with the host code's single pass over the slice. The matrix
checksums are the matrix-core sweep's, whose numpy reference lives in
tests/test_nodeagent_mfmasweep.py.

CPU: exported symbols, the host reference against numpy, the verify and its
attribution of bad waves to role and unit, argument errors, and
check()/report/CLI/chart/docs behaviour against a Python stand-in for the
native library.
GPU (@pytest.mark.gpu, device 0): all checksums at the smallest shapes that
can go wrong, in both dtypes, each role alone, the matrix-core sweep's own
checksums, record sanity, the in-kernel comparison on one flipped word (a data
mismatch in the test's own tensor; nothing on the GPU is provoked), the
default sweep once, and check() end to end.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

# torch first, before any test loads the agent library: see the note at the
# top of test_nodeagent_memtest.py (one HIP runtime per process — torch's).
try:
    import torch
except ImportError:  # CPU-only environment: the GPU tests cannot run there
    torch = None

from gpu_provisioner_amd import nodeagent
from tests.test_nodeagent_mfmasweep import FakeLib as MfmaFakeLib
from tests.test_nodeagent_mfmasweep import ref_checksum as ref_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
U64 = np.uint64
SEED = getattr(nodeagent, "DEFAULT_LOAD_SWEEP_SEED", 0)
GRANULE = 16384
NO_OFFSET = (1 << 64) - 1


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


def ref_slice(seed, workgroup, slice_bytes):
    """The memory image of one workgroup's slice: (lo, hi) per 16-byte vector,
    the memtest pattern at the region-relative vector index."""
    vecs = slice_bytes // 16
    with np.errstate(over="ignore"):
        first = (workgroup * vecs + seed * G) & M64
        h = _mix64(U64(first) + np.arange(vecs, dtype=U64))
        return h, ~((h << U64(32)) | (h >> U64(32)))


@functools.lru_cache(maxsize=None)
def ref_stream(seed, workgroup, slice_bytes, passes):
    """The four stream checksums of one workgroup, wave by wave and step by step."""
    lo, hi = ref_slice(seed, workgroup, slice_bytes)
    lane = np.arange(64)
    out = []
    for q in range(4):
        c = np.zeros(64, dtype=U64)
        for _ in range(passes):
            for j in range(slice_bytes // 16 // 1024):
                lds = np.zeros((4 * 4096 // 16, 2), dtype=U64)  # the workgroup's 16 KiB, as vectors
                for k in range(4):
                    i = j * 1024 + k * 256 + q * 64 + lane
                    slot = (q * 4096 + k * 1024 + lane * 16) // 16
                    lds[slot, 0], lds[slot, 1] = lo[i], hi[i]
                for k in range(4):
                    back = (q * 4096 + k * 1024 + ((lane + 17) & 63) * 16) // 16
                    with np.errstate(over="ignore"):
                        c += lds[back, 0] * U64(G) + lds[back, 1]
        out.append(int(c.sum(dtype=U64)))
    return out


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------

SYMBOLS = ("na_load_sweep_stream_expected", "na_load_sweep_run", "na_load_sweep_verify",
           "na_load_sweep")


def test_library_exports_load_sweep_symbols():
    lib = ctypes.CDLL(_ensure_lib())
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing symbol {sym}"


def test_constants():
    assert SEED.to_bytes(8, "big") == b"MI355XLD"
    assert nodeagent.LOAD_SWEEP_GRANULE == GRANULE == 256 * 4 * 16
    assert nodeagent.LOAD_SWEEP_MAX_BYTES == 16 << 20
    # plain classes over the matrix-core sweep's and the memtest's structs
    assert not issubclass(nodeagent.LoadSweepResult, ctypes.Structure)
    with open(os.path.join(ROOT, "nodeagent", "nodeagent.h")) as f:
        header = f.read()
    for macro in ("NA_LOAD_GRANULE 16384", "NA_LOAD_MAX_BYTES (16 << 20)"):
        assert f"#define {macro}" in header, macro


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


BIG_SEED = (1 << 40) + 9
BIG_WG = (1 << 33) + 5


@pytest.mark.parametrize("seed", [7, SEED, BIG_SEED])
@pytest.mark.parametrize("slice_bytes", [GRANULE, 3 * GRANULE])
def test_stream_expected_matches_reference(cpu_agent, seed, slice_bytes):
    for workgroup in (0, 5, BIG_WG):
        for passes in (1, 3):
            want = ref_stream(seed, workgroup, slice_bytes, passes)
            assert cpu_agent.load_sweep_stream_expected(workgroup, slice_bytes, passes, seed) == want


def test_stream_expected_known_answer(cpu_agent):
    want = ref_stream(SEED, 5, 3 * GRANULE, 3)
    assert [f"{x:#018x}" for x in want] == KNOWN
    assert cpu_agent.load_sweep_stream_expected(5, 3 * GRANULE, 3) == want


KNOWN = ["0x33ec378f272c31d5", "0xfbd43a093666de28", "0x730c2ac3cda36116", "0xc8229f1096204a18"]


def test_stream_reference_properties():
    a = ref_stream(SEED, 5, 3 * GRANULE, 1)
    assert len(set(a)) == 4  # every wave reads its own quarter
    # passes multiply, mod 2^64
    assert ref_stream(SEED, 5, 3 * GRANULE, 3) == [3 * x & M64 for x in a]
    # the four waves together read the whole slice once per pass
    lo, hi = ref_slice(SEED, 5, 3 * GRANULE)
    with np.errstate(over="ignore"):
        assert sum(a) & M64 == int((lo * U64(G) + hi).sum(dtype=U64))
    # region-relative indices: workgroup 5's slice is part of a longer workgroup 1's
    assert all(x != y for x, y in zip(a, ref_stream(SEED, 4, 3 * GRANULE, 1)))
    assert all(x != y for x, y in zip(a, ref_stream(SEED + 1, 5, 3 * GRANULE, 1)))


def test_stream_expected_takes_64_bit_seed_and_workgroup(cpu_agent):
    m32 = (1 << 32) - 1
    got = cpu_agent.load_sweep_stream_expected(BIG_WG, GRANULE, 1, BIG_SEED)
    assert got == ref_stream(BIG_SEED, BIG_WG, GRANULE, 1)
    assert got != cpu_agent.load_sweep_stream_expected(BIG_WG & m32, GRANULE, 1, BIG_SEED)
    assert got != cpu_agent.load_sweep_stream_expected(BIG_WG, GRANULE, 1, BIG_SEED & m32)


def test_stream_expected_argument_errors(cpu_agent):
    out = (ctypes.c_uint64 * 4)()
    for slice_bytes, passes, ptr, n in [
            (0, 1, out, 4), (GRANULE - 16, 1, out, 4), (GRANULE + 4096, 1, out, 4),
            ((16 << 20) + GRANULE, 1, out, 4), (-GRANULE, 1, out, 4), (GRANULE, 0, out, 4),
            (GRANULE, -1, out, 4), (GRANULE, 1, None, 4), (GRANULE, 1, out, 3)]:
        rc = cpu_agent.lib.na_load_sweep_stream_expected(1, 0, slice_bytes, passes, ptr, n)
        assert rc == nodeagent.NA_ERR_ARG, (slice_bytes, passes, n)
        assert "na_load_sweep_stream_expected" in cpu_agent._err()
    with pytest.raises(nodeagent.NodeAgentError):
        cpu_agent.load_sweep_stream_expected(0, GRANULE + 16, 1)


def _unit_of(wave):
    """A made-up placement: the four waves of a role on the four SIMDs of one CU."""
    u = wave // 4
    return (u % 8, (u // 8) % 4, (u // 32) % 2, (u // 64) % 16, wave % 4)


OUTER, SLICE, PASSES = 2, 2 * GRANULE, 2


def _records(workgroups, outer=OUTER, slice_bytes=SLICE, passes=PASSES, seed=SEED):
    """The records of both roles as a clean GPU would leave them; a role that
    is off leaves zeros."""
    n = 4 * workgroups
    matrix, stream = (nodeagent.MfmaRecord * n)(), (nodeagent.MfmaRecord * n)()
    for i in range(n):
        if outer:
            r = matrix[i]
            r.checksum, r.cycles, r.realtime, r.wave = ref_matrix(seed, i, outer), 2400, 100, i
            r.xcc, r.se, r.sh, r.cu, r.simd = _unit_of(i)
        if passes:
            r = stream[i]
            r.checksum = ref_stream(seed, i // 4, slice_bytes, passes)[i % 4]
            r.cycles, r.realtime, r.wave = 2300, 100, i
            r.xcc, r.se, r.sh, r.cu, r.simd = _unit_of(i)
    return matrix, stream


def _verify(agent, matrix, stream, outer=OUTER, slice_bytes=SLICE, passes=PASSES, seed=SEED):
    return agent.load_sweep_verify(matrix, stream, outer, slice_bytes, passes, seed)


def test_verify_clean_records(cpu_agent):
    matrix, stream = _records(6)
    rc, res = _verify(cpu_agent, matrix, stream)
    assert rc == nodeagent.NA_OK and res.ok, cpu_agent._err()
    assert isinstance(res, nodeagent.LoadSweepResult)
    for role in (res.matrix, res.stream):
        assert (role.waves, role.bad_waves, role.units_seen, role.bad_units) == (24, 0, 6, 0)
        assert role.first_bad_wave == nodeagent.NO_BAD_WAVE and role.bad_simds == []
    assert res.matrix.clock_mhz == pytest.approx(2400.0)
    assert res.stream.clock_mhz == pytest.approx(2300.0)
    # the same records do not verify under other counts, another seed or size
    assert _verify(cpu_agent, matrix, stream, outer=3)[1].matrix.bad_waves == 24
    assert _verify(cpu_agent, matrix, stream, outer=3)[1].stream.ok
    assert _verify(cpu_agent, matrix, stream, passes=3)[1].stream.bad_waves == 24
    assert _verify(cpu_agent, matrix, stream, passes=3)[1].matrix.ok
    assert _verify(cpu_agent, matrix, stream, slice_bytes=GRANULE)[1].stream.bad_waves == 24
    other = _verify(cpu_agent, matrix, stream, seed=SEED + 1)[1]
    assert (other.matrix.bad_waves, other.stream.bad_waves) == (24, 24)


@pytest.mark.parametrize("role", ["matrix", "stream"])
def test_verify_one_corrupted_checksum_names_wave_role_and_unit(cpu_agent, role):
    matrix, stream = _records(6)
    wave = 13 if role == "matrix" else 18
    (matrix if role == "matrix" else stream)[wave].checksum ^= 1 << 33
    rc, res = _verify(cpu_agent, matrix, stream)
    assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
    bad, good = (res.matrix, res.stream) if role == "matrix" else (res.stream, res.matrix)
    assert good.ok and good.bad_simds == []
    assert (bad.bad_waves, bad.bad_units, bad.first_bad_wave) == (1, 1, wave)
    assert bad.bad_simds == [_unit_of(wave)]
    name = nodeagent.mfma_unit_name(_unit_of(wave))
    err = cpu_agent._err()
    assert f"first {role} wave {wave} on {name}" in err and "under combined load" in err
    counts = "1 of 24 matrix waves and 0 of 24 stream" if role == "matrix" else \
        "0 of 24 matrix waves and 1 of 24 stream"
    assert counts in err
    text = res.describe()
    assert f"{role} waves failed under combined load" in text and "simd" in text
    assert nodeagent.mfma_unit_name(_unit_of(wave)[:4]) in text
    assert ("matrix waves" in text) == (role == "matrix")


def test_verify_unwritten_and_misplaced_records_are_bad(cpu_agent):
    matrix, stream = _records(6)
    ctypes.memset(ctypes.byref(stream, 9 * ctypes.sizeof(nodeagent.MfmaRecord)), 0xFF,
                  ctypes.sizeof(nodeagent.MfmaRecord))
    rc, res = _verify(cpu_agent, matrix, stream)
    assert rc == nodeagent.NA_ERR_VERIFY and res.matrix.ok
    assert (res.stream.bad_waves, res.stream.first_bad_wave) == (1, 9)
    assert "first stream wave 9 on " in cpu_agent._err()
    # two records that changed places: right checksums of the wrong waves
    matrix, stream = _records(6)
    for field, _type in nodeagent.MfmaRecord._fields_:
        a, b = getattr(matrix[4], field), getattr(matrix[7], field)
        setattr(matrix[4], field, b), setattr(matrix[7], field, a)
    rc, res = _verify(cpu_agent, matrix, stream)
    assert rc == nodeagent.NA_ERR_VERIFY and res.stream.ok
    assert (res.matrix.bad_waves, res.matrix.bad_units, res.matrix.first_bad_wave) == (2, 1, 4)
    # the right checksum under the wrong index alone is as bad
    matrix, stream = _records(6)
    stream[10].wave = 11
    rc, res = _verify(cpu_agent, matrix, stream)
    assert rc == nodeagent.NA_ERR_VERIFY and res.stream.first_bad_wave == 10
    # matrix failures are named first when both roles have some
    matrix[20].checksum += 1
    rc, res = _verify(cpu_agent, matrix, stream)
    assert "1 of 24 matrix waves and 1 of 24 stream waves" in cpu_agent._err()
    assert "first matrix wave 20 on " in cpu_agent._err()
    assert "matrix waves failed" in res.describe() and "stream waves failed" in res.describe()


@pytest.mark.parametrize("off", ["matrix", "stream"])
def test_verify_a_role_that_is_off_must_be_all_zero(cpu_agent, off):
    outer, passes = (0, PASSES) if off == "matrix" else (OUTER, 0)
    matrix, stream = _records(3, outer=outer, passes=passes)
    rc, res = _verify(cpu_agent, matrix, stream, outer=outer, passes=passes)
    assert rc == nodeagent.NA_OK and res.ok, cpu_agent._err()
    idle, busy = (res.matrix, res.stream) if off == "matrix" else (res.stream, res.matrix)
    assert (idle.waves, idle.units_seen, idle.clock_mhz) == (12, 0, 0.0)
    assert (busy.waves, busy.units_seen) == (12, 3)
    recs = matrix if off == "matrix" else stream
    for field in ("checksum", "cycles", "realtime", "wave", "simd"):
        setattr(recs[5], field, 1)
        rc, res = _verify(cpu_agent, matrix, stream, outer=outer, passes=passes)
        assert rc == nodeagent.NA_ERR_VERIFY, field
        idle = res.matrix if off == "matrix" else res.stream
        assert (idle.bad_waves, idle.first_bad_wave) == (1, 5)
        assert f"first {off} wave 5 on " in cpu_agent._err()
        setattr(recs[5], field, 0)
    # the records of a full run do not pass for one with a role off
    matrix, stream = _records(3)
    rc, res = _verify(cpu_agent, matrix, stream, outer=outer, passes=passes)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.matrix if off == "matrix" else res.stream).bad_waves == 12


def test_verify_lists_a_bounded_number_of_units(cpu_agent):
    limit = nodeagent.MFMA_SWEEP_MAX_LISTED
    workgroups = limit + 3
    matrix, stream = _records(workgroups, outer=1, slice_bytes=GRANULE, passes=1)
    for i in range(0, 4 * workgroups, 4):
        stream[i].checksum ^= 1
    rc, res = cpu_agent.load_sweep_verify(matrix, stream, 1, GRANULE, 1)
    assert rc == nodeagent.NA_ERR_VERIFY and res.matrix.ok
    assert (res.stream.bad_waves, res.stream.bad_units) == (workgroups, workgroups)
    assert res.stream.bad_simds == [_unit_of(4 * i) for i in range(limit)]
    assert ", ..." in res.describe()


def test_argument_errors_before_any_hip_call(cpu_agent):
    lib = cpu_agent.lib
    recs, recs2 = (nodeagent.MfmaRecord * 8)(), (nodeagent.MfmaRecord * 8)()
    mem, ms = nodeagent._MemtestResultC(), ctypes.c_double(0)
    res, res2 = nodeagent._MfmaSweepResultC(), nodeagent._MfmaSweepResultC()
    ptr = (1 << 40) + 16  # only printed, never followed

    def run(dtype=0, workgroups=2, outer=1, region=ptr, slice_bytes=GRANULE, passes=1,
            matrix=recs, stream=recs2, n_out=8, mem_p=ctypes.byref(mem)):
        return lib.na_load_sweep_run(0, dtype, workgroups, outer, region, slice_bytes, passes, SEED,
                                     matrix, stream, n_out, mem_p, ctypes.byref(ms))

    for kw, said in [
            (dict(slice_bytes=GRANULE + 4096), "slice_bytes a multiple of 16384"),
            (dict(slice_bytes=GRANULE - 16), "slice_bytes a multiple of 16384"),
            (dict(slice_bytes=0), "(got 0)"),
            (dict(slice_bytes=(16 << 20) + GRANULE), f"up to {16 << 20}"),
            (dict(outer=0, passes=0), "outer and passes are both 0"),
            (dict(dtype=2), "dtype 0 (bf16) or 1 (fp8) (got 2)"),
            (dict(dtype=-1), "(got -1)"),
            (dict(workgroups=0), "workgroups in 1.."),
            (dict(workgroups=(1 << 20) + 1, n_out=1 << 40), "workgroups in 1.."),
            (dict(outer=-1), "outer in 0.."), (dict(outer=(1 << 22) + 1), "outer in 0.."),
            (dict(passes=-1), "passes in 0.."), (dict(passes=1025), "passes in 0..1024"),
            (dict(n_out=7), "n_out 7"), (dict(workgroups=3, n_out=8), "n_out 8"),
            (dict(region=None), "16-byte aligned region"),
            (dict(region=ptr + 8), f"region ({ptr + 8:#x})"),
            (dict(matrix=None), "matrix (nil)"), (dict(stream=None), "stream (nil)"),
            (dict(mem_p=None), "mem (nil)")]:
        assert run(**kw) == nodeagent.NA_ERR_ARG, kw
        assert "na_load_sweep_run: " in cpu_agent._err() and said in cpu_agent._err(), kw

    def verify(matrix=recs, stream=recs2, n=8, outer=1, slice_bytes=GRANULE, passes=1,
               out=ctypes.byref(res), out2=ctypes.byref(res2)):
        return lib.na_load_sweep_verify(matrix, stream, n, outer, slice_bytes, passes, SEED, out,
                                        out2)

    for kw in [dict(matrix=None), dict(stream=None), dict(n=0), dict(n=6), dict(n=-4),
               dict(outer=-1), dict(passes=-1), dict(passes=1025), dict(outer=0, passes=0),
               dict(slice_bytes=GRANULE + 16), dict(slice_bytes=0),
               dict(slice_bytes=(16 << 20) + GRANULE), dict(out=None), dict(out2=None)]:
        assert verify(**kw) == nodeagent.NA_ERR_ARG, kw
        assert "na_load_sweep_verify: " in cpu_agent._err()
    assert cpu_agent.load_sweep_verify(recs, recs2, 0, GRANULE, 0)[0] == nodeagent.NA_ERR_ARG

    tflops, gbs, overlap = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)

    def sweep(dtype=0, workgroups=0, outer=0, slice_bytes=0, passes=0, out=ctypes.byref(res),
              out2=ctypes.byref(res2), mem_p=ctypes.byref(mem)):
        return lib.na_load_sweep(0, dtype, workgroups, outer, slice_bytes, passes, SEED, out, out2,
                                 mem_p, ctypes.byref(tflops), ctypes.byref(gbs),
                                 ctypes.byref(overlap))

    for kw in [dict(dtype=2), dict(workgroups=-1), dict(workgroups=(1 << 20) + 1), dict(outer=-1),
               dict(outer=(1 << 22) + 1), dict(slice_bytes=100), dict(slice_bytes=GRANULE + 4096),
               dict(slice_bytes=(16 << 20) + GRANULE), dict(passes=-1), dict(passes=1025),
               dict(out=None), dict(out2=None), dict(mem_p=None)]:
        assert sweep(**kw) == nodeagent.NA_ERR_ARG, kw
        assert "na_load_sweep: " in cpu_agent._err()
    with pytest.raises(nodeagent.NodeAgentError, match="dtype 'fp4'"):
        cpu_agent.load_sweep_run(0, ptr, dtype="fp4")
    with pytest.raises(nodeagent.NodeAgentError, match="both 0"):
        cpu_agent.load_sweep_run(0, ptr, outer=0, passes=0)


# -- check() against a Python stand-in library --------------------------------

SICK = (5, 2, 1, 9)


class FakeLib(MfmaFakeLib):
    """The matrix-core sweep's stand-in plus na_load_sweep. ``load``: {dev:
    "matrix" | "stream" | "words" | "slow_tflops" | "slow_gbs" | "fewer" |
    "noroom"}; default clean. A sick GPU has one CU whose waves of that role
    compute wrong; "words" is a mismatch only the kernel's comparison saw."""

    def __init__(self, ngpu=1, load=None, **kw):
        super().__init__(ngpu=ngpu, **kw)
        self.load_calls = []
        load = load or {}

        def na_load_sweep(dev, dtype, workgroups, outer, slice_bytes, passes, seed, res_m, res_s,
                          mem, tflops, gbs, overlap):
            self.load_calls.append(
                (dev, dtype, workgroups, outer, slice_bytes.value, passes, seed.value))
            kind = load.get(dev, "ok")
            if kind == "noroom":
                self.error = (b"na_load_sweep: the region of 4294967296 bytes (1024 workgroups x "
                              b"4194304) does not fit: 1073741824 bytes of device memory are free "
                              b"and the sweep takes at most half")
                return nodeagent.NA_ERR_ARG
            for r, mhz in ((res_m._obj, 2188.44), (res_s._obj, 2187.0)):
                r.waves, r.units_seen, r.clock_mhz = 4096, 255 if kind == "fewer" else 256, mhz
                r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            m = mem._obj
            m.bytes_tested, m.bad_words, m.first_bad_offset, m.xor_mask = 1 << 32, 0, NO_OFFSET, 0
            tflops._obj.value = 1.5 if kind == "slow_tflops" else 2051.26
            gbs._obj.value = 2.5 if kind == "slow_gbs" else 3987.66
            overlap._obj.value = 0.9312
            if kind == "words":
                m.bad_words, m.first_bad_offset, m.xor_mask = 3, 0x12345678, 0x0400
                return nodeagent.NA_ERR_VERIFY
            if kind not in ("matrix", "stream"):
                return 0
            r = res_m._obj if kind == "matrix" else res_s._obj
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 8, 1, 404, 2
            for k, simd in enumerate((1, 3)):
                r.bad_list[k][:] = SICK + (simd,)
            r.first_bad_unit[:] = SICK + (1,)
            return nodeagent.NA_ERR_VERIFY

        self.na_load_sweep = na_load_sweep


def _agent(monkeypatch, **kw):
    monkeypatch.setattr(nodeagent, "MIN_LOAD_SWEEP_TFLOPS", 1400.0)
    monkeypatch.setattr(nodeagent, "MIN_LOAD_SWEEP_GBS", 2800.0)
    fake = FakeLib(**kw)
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fake)
    return nodeagent.NodeAgent(), fake


FIELDS = ("load_sweep_tflops", "load_sweep_gbs", "load_sweep_clock_mhz", "load_sweep_overlap",
          "load_sweep_units_seen", "load_sweep_bad_waves", "load_sweep_bad_words",
          "load_sweep_skipped")
NOT_RUN = (0.0, 0.0, 0.0, 0.0, 0, 0, 0, "")


def _sweep_fields(g):
    return tuple(getattr(g, name) for name in FIELDS)


def test_check_default_never_runs_sweep(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check()
    assert fake.load_calls == [] and fake.sweep_calls == []
    assert report.healthy, report.problems
    assert _sweep_fields(report.gpus[0]) == NOT_RUN
    assert _sweep_fields(nodeagent.GPUReport(index=0)) == NOT_RUN
    # the matrix-core sweep's flag does not reach it
    assert agent.check(mfma_sweep=True).healthy and fake.load_calls == []
    # the stand-ins of the other sweeps' tests have no load sweep at all
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: MfmaFakeLib())
    assert nodeagent.NodeAgent().check(mfma_sweep=True).healthy


def test_check_clean_sweep_populates_fields(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check(load_sweep=True)
    assert fake.load_calls == [(0, 0, 0, 0, 0, 0, SEED)] and fake.sweep_calls == []
    g = report.gpus[0]
    assert report.healthy and g.healthy, report.problems
    assert _sweep_fields(g) == (2051.3, 3987.7, 2188.4, 0.931, 256, 0, 0, "")
    assert nodeagent.node_condition_from_report(report)["status"] == "True"


def test_check_units_seen_below_cus_is_reported_not_a_problem(monkeypatch):
    agent, _ = _agent(monkeypatch, load={0: "fewer"})
    report = agent.check(load_sweep=True)
    assert report.gpus[0].load_sweep_units_seen == 255 < report.gpus[0].cus
    assert report.healthy, report.problems


@pytest.mark.parametrize("role", ["matrix", "stream"])
def test_check_eight_gpus_one_wrong_under_load(monkeypatch, role):
    agent, fake = _agent(monkeypatch, ngpu=8, load={3: role})
    report = agent.check(expect_gpus=8, load_sweep=True)
    assert [c[0] for c in fake.load_calls] == list(range(8))
    assert report.problems == [
        f"gpu3: load sweep: {role} waves failed under combined load: 8 of 4096 waves wrong on "
        "1 CU(s): xcc5.se2.sh1.cu9 simd 1,3"
    ]
    assert not report.healthy
    assert [g.healthy for g in report.gpus] == [i != 3 for i in range(8)]
    assert [g.load_sweep_bad_waves for g in report.gpus] == [8 * (i == 3) for i in range(8)]
    cond = nodeagent.node_condition_from_report(report)
    assert cond["status"] == "False" and "xcc5.se2.sh1.cu9" in cond["message"]
    assert role in cond["message"] and "under combined load" in cond["message"]


def test_check_in_kernel_mismatch_is_a_problem(monkeypatch):
    agent, _ = _agent(monkeypatch, load={0: "words"})
    report = agent.check(load_sweep=True)
    g = report.gpus[0]
    assert g.problems == [
        "load sweep: stream comparison: 3 bad 64-bit words in 4294967296 bytes, first at offset "
        "0x12345678, failing bits 0x400"
    ]
    assert (g.load_sweep_bad_words, g.load_sweep_bad_waves) == (3, 0)
    assert nodeagent.node_condition_from_report(report)["status"] == "False"


def test_check_low_rates_flag_problems(monkeypatch):
    agent, _ = _agent(monkeypatch, load={0: "slow_tflops"})
    report = agent.check(load_sweep=True)
    assert report.gpus[0].problems == ["load sweep 1.5 TFLOP/s below floor 1400.0"]
    agent, _ = _agent(monkeypatch, load={0: "slow_gbs"})
    report = agent.check(load_sweep=True)
    assert report.gpus[0].problems == ["load sweep 2.5 GB/s below floor 2800.0"]
    assert nodeagent.node_condition_from_report(report)["status"] == "False"
    # 0 disables a floor
    monkeypatch.setattr(nodeagent, "MIN_LOAD_SWEEP_GBS", 0.0)
    assert agent.check(load_sweep=True).healthy


def test_check_region_that_does_not_fit_is_a_recorded_skip(monkeypatch):
    agent, fake = _agent(monkeypatch, load={0: "noroom"})
    report = agent.check(load_sweep=True)
    g = report.gpus[0]
    assert len(fake.load_calls) == 1
    assert report.healthy and g.healthy and g.problems == []
    assert "does not fit" in g.load_sweep_skipped and "1073741824 bytes" in g.load_sweep_skipped
    assert _sweep_fields(g)[:-1] == NOT_RUN[:-1]
    assert nodeagent.node_condition_from_report(report)["status"] == "True"


def test_floors_are_derived_from_the_profile():
    """0.70 x the median of the profile's per-process figures."""
    with open(os.path.join(ROOT, "profiles", "load_sweep_mi355x.txt")) as f:
        lines = f.read().splitlines()
    for key, floor in (("tflops ", nodeagent.MIN_LOAD_SWEEP_TFLOPS),
                       ("gbs ", nodeagent.MIN_LOAD_SWEEP_GBS)):
        runs = [float(x) for line in lines if line.startswith(key) for x in line.split()[1:]]
        assert len(runs) >= 5
        assert floor > 0
        assert floor == pytest.approx(0.70 * float(np.median(runs)), abs=0.06)


def test_cli_flag_reaches_check(monkeypatch, capsys):
    _, fake = _agent(monkeypatch)
    assert nodeagent.main(["--load-sweep"]) == 0
    assert [c[0] for c in fake.load_calls] == [0] and fake.sweep_calls == []
    assert json.loads(capsys.readouterr().out)["gpus"][0]["load_sweep_units_seen"] == 256
    _, fake = _agent(monkeypatch)
    assert nodeagent.main([]) == 0
    assert fake.load_calls == []
    capsys.readouterr()


def test_chart_passes_load_sweep_only_when_true():
    import yaml

    chart = os.path.join(ROOT, "charts", "gpu-provisioner-amd")
    with open(os.path.join(chart, "values.yaml")) as f:
        values = yaml.safe_load(f)
    assert values["nodeAgent"]["loadSweep"] is False
    with open(os.path.join(chart, "templates", "amd-gpu-node-stack.yaml")) as f:
        text = f.read()
    start = text.index("{{- if .Values.nodeAgent.loadSweep }}")
    end = text.index("{{- end }}", start)
    assert "--load-sweep \\" in text[start:end]
    assert text.count("--load-sweep") == 1  # nowhere outside the guard


def test_docs_cover_every_new_report_field():
    with open(os.path.join(ROOT, "docs", "METRICS.md")) as f:
        metrics = f.read()
    for name in FIELDS:
        assert f"| `{name}` |" in metrics, name
        assert hasattr(nodeagent.GPUReport(index=0), name)
    for doc in ("DESIGN.md", "OPERATIONS.md"):
        with open(os.path.join(ROOT, "docs", doc)) as f:
            assert "--load-sweep" in f.read(), doc
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "--load-sweep" in f.read()


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


_regions = {}


def _region(agent, workgroups, slice_bytes, seed=SEED):
    """A pattern-filled region per distinct shape, shared by the tests; read-only."""
    key = (workgroups, slice_bytes, seed)
    if key not in _regions:
        words = torch.empty(workgroups * slice_bytes // 8, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        assert agent.memtest_fill(0, words.data_ptr(), workgroups * slice_bytes, seed) == 0
        _regions[key] = words
    return _regions[key]


_runs = {}


def _run(agent, workgroups, outer, slice_bytes, passes, dtype="bf16"):
    """One launch per distinct shape, shared by the tests; read-only."""
    key = (workgroups, outer, slice_bytes, passes, dtype)
    if key not in _runs:
        region = _region(agent, workgroups, slice_bytes)
        torch.cuda.synchronize()
        _runs[key] = agent.load_sweep_run(0, region.data_ptr(), workgroups, outer, slice_bytes,
                                          passes, SEED, dtype)
    return _runs[key]


def _want(workgroups, outer, slice_bytes, passes):
    n = 4 * workgroups
    matrix = [ref_matrix(SEED, i, outer) if outer else 0 for i in range(n)]
    stream = [ref_stream(SEED, i // 4, slice_bytes, passes)[i % 4] if passes else 0
              for i in range(n)]
    return matrix, stream


def _assert_run_matches(run, workgroups, outer, slice_bytes, passes):
    matrix, stream, mem, _ms = run
    want_m, want_s = _want(workgroups, outer, slice_bytes, passes)
    got_m, got_s = [r.checksum for r in matrix], [r.checksum for r in stream]
    print(f"{workgroups} workgroups, outer {outer}, {slice_bytes} bytes x {passes}: matrix",
          [f"{x:#x}" for x in got_m], "stream", [f"{x:#x}" for x in got_s], "mem", mem)
    assert got_m == want_m
    assert got_s == want_s
    assert mem.bad_words == 0 and mem.first_bad_offset == NO_OFFSET and mem.xor_mask == 0


@pytest.mark.gpu
def test_gpu_smallest_shape(agent):
    _assert_run_matches(_run(agent, 1, 1, GRANULE, 1), 1, 1, GRANULE, 1)


@pytest.mark.gpu
def test_gpu_where_it_can_first_go_wrong_in_both_dtypes(agent):
    """Three workgroups, the pipelined fold loop's body, a second step and a second pass."""
    shape = (3, 2, 2 * GRANULE, 2)
    bf16, fp8 = _run(agent, *shape, dtype="bf16"), _run(agent, *shape, dtype="fp8")
    _assert_run_matches(bf16, *shape)
    _assert_run_matches(fp8, *shape)
    assert [r.checksum for r in bf16[0]] == [r.checksum for r in fp8[0]]
    rc, res = agent.load_sweep_verify(bf16[0], bf16[1], 2, 2 * GRANULE, 2)
    assert rc == nodeagent.NA_OK and res.ok, agent._err()


@pytest.mark.gpu
def test_gpu_each_role_alone(agent):
    workgroups, slice_bytes = 3, 2 * GRANULE
    both = _run(agent, workgroups, 3, slice_bytes, 2)
    _assert_run_matches(both, workgroups, 3, slice_bytes, 2)
    zero = bytes(ctypes.sizeof(nodeagent.MfmaRecord))
    for outer, passes in ((3, 0), (0, 2)):
        run = _run(agent, workgroups, outer, slice_bytes, passes)
        _assert_run_matches(run, workgroups, outer, slice_bytes, passes)
        idle, busy, ref = (run[1], run[0], both[0]) if passes == 0 else (run[0], run[1], both[1])
        assert all(bytes(r) == zero for r in idle)
        assert [r.checksum for r in busy] == [r.checksum for r in ref]
        assert all(r.cycles > 0 and r.realtime > 0 for r in busy)
        rc, res = agent.load_sweep_verify(run[0], run[1], outer, slice_bytes, passes)
        assert rc == nodeagent.NA_OK and res.ok, agent._err()


@pytest.mark.gpu
def test_gpu_same_chain_as_the_mfma_sweep(agent):
    matrix = _run(agent, 3, 2, 2 * GRANULE, 2)[0]
    torch.cuda.synchronize()
    alone, _ms = agent.mfma_sweep_run(0, "bf16", 3, 2, SEED)
    assert [r.checksum for r in matrix] == [r.checksum for r in alone]
    assert [r.wave for r in matrix] == [r.wave for r in alone] == list(range(12))


@pytest.mark.gpu
def test_gpu_record_sanity(agent):
    workgroups = 3
    matrix, stream, _mem, _ms = _run(agent, workgroups, 2, 2 * GRANULE, 2)
    assert [r.wave for r in matrix] == [r.wave for r in stream] == list(range(4 * workgroups))
    spread = 0
    for g in range(workgroups):
        recs = list(matrix[4 * g:4 * g + 4]) + list(stream[4 * g:4 * g + 4])
        for r in recs:
            assert r.cycles > 0 and r.realtime > 0
            assert r.xcc < 8 and r.se < 4 and r.sh < 2 and r.cu < 16 and r.simd < 4
        assert len({(r.xcc, r.se, r.sh, r.cu) for r in recs}) == 1
        spread += len({r.simd for r in matrix[4 * g:4 * g + 4]}) == 4
    print(f"{spread} of {workgroups} workgroups have one matrix wave per SIMD; matrix SIMDs "
          f"{[r.simd for r in matrix]}, stream SIMDs {[r.simd for r in stream]}")


@pytest.mark.gpu
def test_gpu_in_kernel_comparison_sees_one_flipped_word(agent):
    workgroups, outer, slice_bytes = 3, 2, 2 * GRANULE
    vecs = slice_bytes // 16
    # the hi word of a vector of workgroup 1's second step, read by its stream wave 2
    v, mask = vecs + 1024 + 2 * 256 + 2 * 64 + 37, 0x0000_0400_0000_0001
    assert (v // vecs, (v % vecs >> 6) & 3) == (1, 2)
    words = _region(agent, workgroups, slice_bytes).clone()
    words[2 * v + 1] ^= mask
    torch.cuda.synchronize()
    matrix, stream, mem, _ms = agent.load_sweep_run(0, words.data_ptr(), workgroups, outer,
                                                    slice_bytes, 1, SEED)
    print("flipped word:", mem)
    assert mem.bad_words == 1
    assert mem.first_bad_offset == 16 * v + 8 and mem.xor_mask == mask
    rc, res = agent.load_sweep_verify(matrix, stream, outer, slice_bytes, 1)
    assert rc == nodeagent.NA_ERR_VERIFY and res.matrix.ok
    assert (res.stream.bad_waves, res.stream.first_bad_wave) == (1, 1 * 4 + 2)
    want_m, want_s = _want(workgroups, outer, slice_bytes, 1)
    assert [r.checksum for r in matrix] == want_m
    assert [i for i, r in enumerate(stream) if r.checksum != want_s[i]] == [6]
    # the region the other tests share is as it was
    _assert_run_matches(agent.load_sweep_run(0, _region(agent, workgroups, slice_bytes).data_ptr(),
                                             workgroups, outer, slice_bytes, 1, SEED),
                        workgroups, outer, slice_bytes, 1)


_sweeps = []


def _default_sweep(agent):
    if not _sweeps:
        torch.cuda.synchronize()
        _sweeps.append(agent.load_sweep(0))
    return _sweeps[0]


@pytest.mark.gpu
def test_gpu_default_sweep(agent):
    res = _default_sweep(agent)
    _, _, _, cus = agent.device_info(0)
    print(f"load_sweep: {res.tflops:.1f} TFLOP/s and {res.gbs:.1f} GB/s together at "
          f"{res.matrix.clock_mhz:.0f} MHz (stream waves {res.stream.clock_mhz:.0f}), overlap "
          f"{res.overlap:.3f}, {res.matrix.units_seen} of {cus} CUs, {res.matrix.waves} waves per "
          f"role, {res.mem.bytes_tested} bytes")
    assert res.ok, res.describe()
    assert res.matrix.waves == res.stream.waves == 16 * cus
    assert res.matrix.bad_waves == res.stream.bad_waves == res.mem.bad_words == 0
    # one workgroup per CU at a time: every CU takes part (the other sweeps' rule)
    assert res.matrix.units_seen == res.stream.units_seen == cus
    assert 0 < res.overlap <= 1
    assert res.tflops >= nodeagent.MIN_LOAD_SWEEP_TFLOPS > 0
    assert res.gbs >= nodeagent.MIN_LOAD_SWEEP_GBS > 0


@pytest.mark.gpu
def test_gpu_check_with_sweep(agent):
    torch.cuda.synchronize()
    report = agent.check(bw_bytes=1 << 28, load_sweep=True)
    g0 = report.gpus[0]
    assert g0.healthy, g0.problems
    assert nodeagent.node_condition_from_report(report)["status"] == "True"
    assert g0.load_sweep_tflops >= nodeagent.MIN_LOAD_SWEEP_TFLOPS
    assert g0.load_sweep_gbs >= nodeagent.MIN_LOAD_SWEEP_GBS
    assert g0.load_sweep_clock_mhz > 0 and 0 < g0.load_sweep_overlap <= 1
    assert g0.load_sweep_units_seen == g0.cus
    assert (g0.load_sweep_bad_waves, g0.load_sweep_bad_words, g0.load_sweep_skipped) == (0, 0, "")
