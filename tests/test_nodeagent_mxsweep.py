"""Chip-wide MX sweep of the node agent (na_mx_sweep*, nodeagent/mfmasweep.h
on v_mfma_scale_f32_16x16x128_f8f6f4), and check() with the MX checks and
the MX sweep switched on.

The sweep is the matrix-core sweep of test_nodeagent_mfmasweep.py on K = 128.
Arithmetic mod 2^64, G = 0x9E3779B97F4A7C15, mix64 the splitmix64 finaliser.
For global wave w, matrix m (0 = A, 1 = B), fragment t in 0..7, r in 0..15
(row of A / column of B) and k in 0..127:

  idx = (((w*2 + m)*8 + t)*16 + r)*128 + k
  e   = mix64(seed*G + idx)
  A   = ((e >> 40) % 7) - 3          B = ((e >> 40) % 5) - 2

One fold = every A fragment times every B fragment (64 MFMAs, |D| <= 49152,
exact). After each fold, per lane l and for i = 0..3:
c = c*G + (uint64)(int64)D[(l>>4)*4+i][l&15]; the wave checksum is sum_l c_l.
fp4 (E2M1) and fp6 (E2M3) hold the same integers, so they agree.

The reference below is numpy written from this text, independent of the
kernel and of the host code's closed form.

CPU: the host reference against numpy, verify and localisation on host
records, argument errors, and check()/report/CLI behaviour against a Python
stand-in for the native library. GPU (@pytest.mark.gpu, device 0): record
checksums at the smallest shapes that can go wrong, format agreement, and the
default sweep once per format against the bf16 sweep's rate. Only HOST data
is corrupted; nothing on the GPU is provoked.
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
from tests.test_nodeagent_memtest import FakeLib as MemtestFakeLib

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEED = nodeagent.DEFAULT_MX_SWEEP_SEED
K = 128


def _ensure_lib():
    import __graft_entry__ as g

    if not os.path.exists(g.LIB_PATH):
        g.build()
    return g.LIB_PATH


# ---------------------------------------------------------------------------
# numpy reference of the specification
# ---------------------------------------------------------------------------


def _mix64(x):
    x = x.copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def ref_fragments(seed, wave):
    """(A, B): int64 arrays [t][r][k], r = row of A / column of B."""
    m, t, r, k = np.meshgrid(
        np.arange(2, dtype=np.uint64), np.arange(8, dtype=np.uint64),
        np.arange(16, dtype=np.uint64), np.arange(K, dtype=np.uint64), indexing="ij",
    )
    with np.errstate(over="ignore"):
        idx = (((np.uint64(wave) * np.uint64(2) + m) * np.uint64(8) + t) * np.uint64(16) + r) \
            * np.uint64(K) + k
        e = _mix64(np.uint64((seed * G) & M64) + idx) >> np.uint64(40)
    a = (e[0] % np.uint64(7)).astype(np.int64) - 3
    b = (e[1] % np.uint64(5)).astype(np.int64) - 2
    return a, b


@functools.lru_cache(maxsize=None)
def ref_fold(seed, wave):
    """D[row][col] of one fold: every A fragment times every B fragment."""
    a, b = ref_fragments(seed, wave)
    d = np.zeros((16, 16), dtype=np.int64)
    for ta in range(8):
        for tb in range(8):
            d += a[ta] @ b[tb].T
    d.setflags(write=False)
    return d


def ref_checksum(seed, wave, outer):
    """The recurrence as the plain loop over folds."""
    d = ref_fold(seed, wave)
    lane = np.arange(64)
    vals = np.stack([d[(lane >> 4) * 4 + i, lane & 15] for i in range(4)]).view(np.uint64)
    c = np.zeros(64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for _ in range(outer):
            for i in range(4):
                c = c * np.uint64(G) + vals[i]
        return int(c.sum(dtype=np.uint64))


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------

SYMBOLS = ("na_mx_sweep_expected", "na_mx_sweep_run", "na_mx_sweep_verify", "na_mx_sweep")


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


def test_library_exports_mx_sweep_symbols(cpu_agent):
    for sym in SYMBOLS:
        assert hasattr(cpu_agent.lib, sym), f"missing symbol {sym}"
    assert nodeagent.MX_SWEEP_FORMATS == {"fp4": 0, "fp6": 1}


def test_reference_values_and_bounds():
    a, b = ref_fragments(SEED, 3)
    assert a.shape == b.shape == (8, 16, K)
    assert set(np.unique(a)) == set(range(-3, 4)) and set(np.unique(b)) == set(range(-2, 3))
    # the fold is (sum A)(sum B), every element within 128 * 24 * 16
    d = ref_fold(SEED, 3)
    assert np.array_equal(d, a.sum(0) @ b.sum(0).T)
    assert np.abs(d).max() <= 49152
    # waves and seeds get different data, and K = 128 is not the K = 32 sweep
    assert ref_checksum(SEED, 3, 1) != ref_checksum(SEED, 4, 1)
    assert ref_checksum(SEED, 3, 1) != ref_checksum(SEED + 1, 3, 1)


@pytest.mark.parametrize("seed,wave", [(0, 0), (7, 1), (SEED, 5), (SEED, 4095)])
def test_expected_checksum_matches_reference(cpu_agent, seed, wave):
    for outer in (1, 2, 3):
        assert cpu_agent.mx_sweep_expected(wave, outer, seed) == ref_checksum(seed, wave, outer)
    # and is not what the K = 32 sweep expects of the same wave
    assert cpu_agent.mx_sweep_expected(wave, 2, seed) != cpu_agent.mfma_sweep_expected(
        wave, 2, seed)


def test_expected_checksum_argument_errors(cpu_agent):
    out = ctypes.c_uint64(0)
    lib = cpu_agent.lib
    u64 = ctypes.c_ulonglong
    assert lib.na_mx_sweep_expected(u64(1), u64(0), 0, ctypes.byref(out)) == nodeagent.NA_ERR_ARG
    assert cpu_agent._err().startswith("na_mx_sweep_expected: ")
    assert lib.na_mx_sweep_expected(u64(1), u64(0), 1, None) == nodeagent.NA_ERR_ARG


def _unit_of(wave):
    """A made-up placement: four waves per workgroup on one CU, SIMD = wave & 3."""
    wg = wave // 4
    return (wg % 8, (wg // 8) % 4, (wg // 32) % 2, (wg // 64) % 16, wave % 4)


def _records(n, outer, seed=SEED):
    recs = (nodeagent.MfmaRecord * n)()
    for i in range(n):
        r = recs[i]
        r.checksum = ref_checksum(seed, i, outer)
        r.cycles, r.realtime, r.wave = 2_100_000 + i, 100_000, i
        r.xcc, r.se, r.sh, r.cu, r.simd = _unit_of(i)
    return recs


def test_verify_clean_records(cpu_agent):
    recs = _records(12, 2)
    rc, res = cpu_agent.mx_sweep_verify(recs, 2)
    assert rc == nodeagent.NA_OK and res.ok and res.dtype == "fp4"
    assert (res.waves, res.bad_waves, res.units_seen, res.bad_units) == (12, 0, 3, 0)
    assert res.first_bad_wave == nodeagent.NO_BAD_WAVE and res.bad_simds == []
    # the same records do not verify under another fold count or seed, nor as
    # records of the K = 32 sweep
    assert cpu_agent.mx_sweep_verify(recs, 3)[0] == nodeagent.NA_ERR_VERIFY
    assert cpu_agent.mx_sweep_verify(recs, 2, SEED + 1)[1].bad_waves == 12
    assert cpu_agent.mfma_sweep_verify(recs, 2, SEED)[1].bad_waves == 12


@pytest.mark.parametrize("wave,bit", [(0, 0), (7, 63), (11, 31)])
def test_verify_localises_one_flipped_bit(cpu_agent, wave, bit):
    recs = _records(12, 2)
    recs[wave].checksum ^= 1 << bit
    rc, res = cpu_agent.mx_sweep_verify(recs, 2, fmt="fp6")
    assert rc == nodeagent.NA_ERR_VERIFY and not res.ok and res.dtype == "fp6"
    assert (res.bad_waves, res.bad_units, res.first_bad_wave) == (1, 1, wave)
    assert res.bad_simds == [_unit_of(wave)]
    err = cpu_agent._err()
    assert err.startswith("mx sweep: 1 of 12 waves wrong on 1 CU(s), first wave %d " % wave)
    assert nodeagent.mfma_unit_name(_unit_of(wave)) in err


def test_verify_record_in_the_wrong_place_is_bad(cpu_agent):
    recs = _records(8, 1)
    recs[5].wave = 6
    rc, res = cpu_agent.mx_sweep_verify(recs, 1)
    assert rc == nodeagent.NA_ERR_VERIFY and (res.bad_waves, res.first_bad_wave) == (1, 5)


def test_run_argument_errors_before_any_hip_call(cpu_agent):
    lib = cpu_agent.lib
    recs = (nodeagent.MfmaRecord * 8)()
    ms = ctypes.c_double(0)
    seed = ctypes.c_ulonglong(SEED)

    def run(fmt, workgroups, outer, out, n_out, fn=lib.na_mx_sweep_run):
        return fn(0, fmt, workgroups, outer, seed, out, ctypes.c_longlong(n_out),
                  ctypes.byref(ms))

    for args in [(2, 2, 1, recs, 8), (-1, 2, 1, recs, 8), (3, 2, 1, recs, 8), (0, 0, 1, recs, 8),
                 (1, -3, 1, recs, 8), (0, 2, 0, recs, 8), (1, 2, -1, recs, 8),
                 (0, 2, 1, None, 8), (0, 2, 1, recs, 7), (0, 3, 1, recs, 8)]:
        assert run(*args) == nodeagent.NA_ERR_ARG, args
        assert cpu_agent._err().startswith("na_mx_sweep_run: need format 0 (fp4) or 1 (fp6)")
    # the whole sweep rejects the same formats, and the K = 32 sweep still
    # knows no third dtype
    res = nodeagent._MfmaSweepResultC()
    tf = ctypes.c_double(0)
    for fmt in (2, -1):
        assert lib.na_mx_sweep(0, fmt, 1, 1, seed, ctypes.byref(res), ctypes.byref(tf)) \
            == nodeagent.NA_ERR_ARG
    assert run(2, 2, 1, recs, 8, fn=lib.na_mfma_sweep_run) == nodeagent.NA_ERR_ARG
    assert cpu_agent._err().startswith("na_mfma_sweep_run: need dtype 0 (bf16) or 1 (fp8)")
    with pytest.raises(nodeagent.NodeAgentError):
        cpu_agent.mx_sweep_run(0, "fp8")


# -- check() against a Python stand-in library --------------------------------

SICK_CU = (2, 1, 0, 5)
BAD_WORD = b"mx bf6 tile: D[3][5] got 139 want 138"


class FakeLib(MemtestFakeLib):
    """The memtest stand-in plus the MX entry points check() uses.
    ``sweep``: {dev: "sick" | "slow"}; a sick GPU has one CU whose four SIMDs
    compute wrong in both formats. ``bad_kind``: {dev: kind name} whose verify
    fails."""

    def __init__(self, ngpu=1, sweep=None, bad_kind=None):
        super().__init__(ngpu=ngpu)
        self.mx_calls = []
        sweep = sweep or {}
        bad_kind = bad_kind or {}
        names = list(nodeagent.MX_CHECK_KINDS)

        def na_mx_check_run(dev, kind, words, n_words):
            self.mx_calls.append(("run", dev, kind))
            words[0] = dev  # so the verify knows whose words these are
            return 0

        def na_mx_check_verify(kind, words, n_words):
            self.mx_calls.append(("verify", words[0], kind))
            if bad_kind.get(words[0]) == names[kind]:
                self.error = BAD_WORD
                return nodeagent.NA_ERR_VERIFY
            return 0

        def na_mx_sweep(dev, fmt, workgroups, outer, seed, res, tflops):
            self.mx_calls.append(("sweep", dev, fmt, workgroups, outer, seed.value))
            state = sweep.get(dev, "ok")
            r = res._obj
            r.waves, r.units_seen, r.clock_mhz = 4096, 256, 2251.26
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            tflops._obj.value = (0.5 if state == "slow" else 8012.34) * (1 if fmt == 0 else 0.99)
            if state != "sick":
                return 0
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 16, 1, 404, 4
            for simd in range(4):
                r.bad_list[simd][:] = SICK_CU + (simd,)
            r.first_bad_unit[:] = SICK_CU + (0,)
            return nodeagent.NA_ERR_VERIFY

        self.na_mx_check_run = na_mx_check_run
        self.na_mx_check_verify = na_mx_check_verify
        self.na_mx_sweep = na_mx_sweep


def _agent(monkeypatch, **kw):
    fake = FakeLib(**kw)
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fake)
    return nodeagent.NodeAgent(), fake


def _mx_fields(g):
    return (g.mx_checks_run, g.mx_checks_failed, g.mx_sweep_fp4_tflops, g.mx_sweep_fp6_tflops,
            g.mx_sweep_bad_waves)


NOT_RUN = (0, [], 0.0, 0.0, 0)


def test_check_default_calls_nothing_new(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check()
    assert fake.mx_calls == []
    assert report.healthy, report.problems
    assert _mx_fields(report.gpus[0]) == NOT_RUN
    assert _mx_fields(nodeagent.GPUReport(index=0)) == NOT_RUN
    # the new fields come after every earlier one
    fields = list(nodeagent.GPUReport.__dataclass_fields__)
    assert fields[-5:] == ["mx_checks_run", "mx_checks_failed", "mx_sweep_fp4_tflops",
                           "mx_sweep_fp6_tflops", "mx_sweep_bad_waves"]
    assert fields[-6] == "mfma_sweep_bad_waves"
    # a stand-in with no MX function at all passes the default check, with the
    # older options on too
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: MemtestFakeLib())
    assert nodeagent.NodeAgent().check(memtest_bytes=1024).healthy
    assert nodeagent.MIN_MX_SWEEP_TFLOPS >= 0.0


def test_check_with_mx_options_populates_fields(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check(mx_checks=True, mx_sweep=True)
    n = len(nodeagent.MX_CHECK_KINDS)
    assert fake.mx_calls == (
        [(what, 0, kind) for kind in range(n) for what in ("run", "verify")]
        + [("sweep", 0, 0, 0, 0, SEED), ("sweep", 0, 1, 0, 0, SEED)])
    g = report.gpus[0]
    assert report.healthy and g.healthy, report.problems
    assert _mx_fields(g) == (n, [], 8012.3, 7932.2, 0)
    assert nodeagent.node_condition_from_report(report)["status"] == "True"
    # each option alone runs only its own part
    agent, fake = _agent(monkeypatch)
    assert _mx_fields(agent.check(mx_checks=True).gpus[0]) == (n, [], 0.0, 0.0, 0)
    assert {c[0] for c in fake.mx_calls} == {"run", "verify"}
    agent, fake = _agent(monkeypatch)
    assert _mx_fields(agent.check(mx_sweep=True).gpus[0]) == (0, [], 8012.3, 7932.2, 0)
    assert {c[0] for c in fake.mx_calls} == {"sweep"}


def test_check_failing_kind_is_a_problem_with_the_word(monkeypatch):
    agent, fake = _agent(monkeypatch, ngpu=2, bad_kind={1: "bf6"})
    report = agent.check(mx_checks=True)
    assert report.problems == [f"gpu1: MX check bf6 failed: {BAD_WORD.decode()}"]
    assert [g.healthy for g in report.gpus] == [True, False]
    g = report.gpus[1]
    # the kinds after the failing one still ran
    assert (g.mx_checks_run, g.mx_checks_failed) == (len(nodeagent.MX_CHECK_KINDS), ["bf6"])
    assert nodeagent.node_condition_from_report(report)["message"] == report.problems[0]


def test_check_sick_cu_is_named(monkeypatch):
    agent, fake = _agent(monkeypatch, ngpu=8, sweep={3: "sick"})
    report = agent.check(expect_gpus=8, mx_sweep=True)
    assert [c[1:3] for c in fake.mx_calls] == [(d, f) for d in range(8) for f in (0, 1)]
    assert report.problems == [
        f"gpu3: MX sweep {fmt}: 16 of 4096 waves wrong on 1 CU(s): xcc2.se1.sh0.cu5 simd 0,1,2,3"
        for fmt in ("fp4", "fp6")
    ]
    assert [g.healthy for g in report.gpus] == [i != 3 for i in range(8)]
    assert [g.mx_sweep_bad_waves for g in report.gpus] == [32 if i == 3 else 0 for i in range(8)]


def test_check_low_fp4_rate_is_a_problem_once_a_floor_is_set(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_MX_SWEEP_TFLOPS", 5000.0)
    agent, _ = _agent(monkeypatch, sweep={0: "slow"})
    report = agent.check(mx_sweep=True)
    assert report.gpus[0].problems == ["MX sweep fp4 0.5 TFLOP/s below floor 5000.0"]
    agent, _ = _agent(monkeypatch)
    assert agent.check(mx_sweep=True).healthy


def test_cli_flags_reach_check(monkeypatch, capsys):
    _, fake = _agent(monkeypatch)
    assert nodeagent.main(["--mx-checks", "--mx-sweep"]) == 0
    assert [c[0] for c in fake.mx_calls].count("sweep") == 2
    g0 = json.loads(capsys.readouterr().out)["gpus"][0]
    assert g0["mx_checks_run"] == len(nodeagent.MX_CHECK_KINDS) and g0["mx_checks_failed"] == []
    assert g0["mx_sweep_fp4_tflops"] == 8012.3
    _, fake = _agent(monkeypatch)
    assert nodeagent.main([]) == 0
    assert fake.mx_calls == []
    capsys.readouterr()


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


_runs = {}


def _run(agent, fmt, workgroups, outer, seed=SEED):
    """One launch per distinct shape, shared by the tests; read-only."""
    key = (fmt, workgroups, outer, seed)
    if key not in _runs:
        torch.cuda.synchronize()
        _runs[key] = agent.mx_sweep_run(0, fmt, workgroups, outer, seed)[0]
    return _runs[key]


# (1, 1): one workgroup, one fold; (3, 2): wave indexing across workgroups
# and the chaining of folds (the loop is pipelined by one fold, so outer = 1
# and outer = 2 leave it by different paths)
@pytest.mark.gpu
@pytest.mark.parametrize("fmt,workgroups,outer", [("fp4", 1, 1), ("fp4", 3, 2), ("fp6", 3, 2)])
def test_gpu_record_checksums_match_reference(agent, fmt, workgroups, outer):
    recs = _run(agent, fmt, workgroups, outer)
    assert len(recs) == 4 * workgroups
    assert [r.wave for r in recs] == list(range(4 * workgroups))
    for w, r in enumerate(recs):
        assert r.checksum == ref_checksum(SEED, w, outer), f"{fmt} wave {w}: {r.checksum:#x}"
    rc, res = agent.mx_sweep_verify(recs, outer, fmt=fmt)
    assert rc == nodeagent.NA_OK and res.ok, agent._err()


@pytest.mark.gpu
def test_gpu_formats_agree_and_seed_matters(agent):
    fp4 = [r.checksum for r in _run(agent, "fp4", 3, 2)]
    fp6 = [r.checksum for r in _run(agent, "fp6", 3, 2)]
    other = [r.checksum for r in _run(agent, "fp4", 3, 2, seed=7)]
    assert fp4 == fp6
    assert all(a != b for a, b in zip(fp4, other))
    assert other == [ref_checksum(7, w, 2) for w in range(12)]


@pytest.mark.gpu
def test_gpu_default_sweep_and_rate_against_bf16(agent):
    """The default sweep once per format, and the fp4 rate against the bf16
    sweep's measured in the same test: the block-scaled instruction does 4x
    the K of the bf16 one in the same cycles, so anything not above 1x means
    the sweep is not running at the matrix cores' fp4 rate."""
    torch.cuda.synchronize()
    bf16 = agent.mfma_sweep(0, "bf16")
    res = {fmt: agent.mx_sweep(0, fmt) for fmt in ("fp4", "fp6")}
    for fmt, r in res.items():
        print(f"mx_sweep {fmt}: {r.tflops:.1f} TFLOP/s, {r.clock_mhz:.0f} MHz, "
              f"{r.units_seen} CUs, {r.waves} waves, {r.tflops / bf16.tflops:.2f}x bf16 "
              f"({bf16.tflops:.1f} TFLOP/s at {bf16.clock_mhz:.0f} MHz)")
        assert r.ok, r.describe()
        assert r.dtype == fmt and r.bad_waves == 0 and r.bad_simds == []
        assert r.waves == bf16.waves and r.units_seen > 0
        assert 500 < r.clock_mhz < 3500  # a shader clock, in MHz
        assert r.tflops > 0
    assert bf16.ok, bf16.describe()
    assert res["fp4"].tflops > bf16.tflops


@pytest.mark.gpu
def test_gpu_check_with_mx_options(agent):
    torch.cuda.synchronize()
    report = agent.check(bw_bytes=1 << 28, mx_checks=True, mx_sweep=True)
    g0 = report.gpus[0]
    assert g0.healthy, g0.problems
    assert (g0.mx_checks_run, g0.mx_checks_failed) == (len(nodeagent.MX_CHECK_KINDS), [])
    assert g0.mx_sweep_fp4_tflops > 0 and g0.mx_sweep_fp6_tflops > 0
    assert g0.mx_sweep_bad_waves == 0
