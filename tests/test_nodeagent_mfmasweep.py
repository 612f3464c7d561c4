"""Chip-wide matrix-core sweep of the node agent (nodeagent/mfmasweep.h).

The reference for every checksum is the numpy implementation of the
specification below — fragment hash, all 64 fragment products as integer
matmuls, the lane layout, and the checksum recurrence as the plain loop —
written from the specification, independent of the kernel and of the host
code's closed form, and pinned by known answers.

CPU: exported symbols, the host reference against numpy, the verify and its
attribution of bad waves to units, argument errors, and check()/report/
condition/CLI/chart behaviour against a Python stand-in for the native
library.
GPU (@pytest.mark.gpu, device 0): record checksums at the smallest shapes
that can go wrong, dtype agreement, record sanity, localisation on the GPU's
own records (only HOST data is corrupted; nothing on the GPU is provoked),
the default sweep once per dtype, and the end-to-end paths.
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
from gpu_provisioner_amd.apis import v1 as karpv1
from tests.test_nodeagent_memtest import FakeLib as MemtestFakeLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEED = nodeagent.DEFAULT_MFMA_SWEEP_SEED


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
        np.arange(16, dtype=np.uint64), np.arange(32, dtype=np.uint64), indexing="ij",
    )
    with np.errstate(over="ignore"):
        idx = (((np.uint64(wave) * np.uint64(2) + m) * np.uint64(8) + t) * np.uint64(16) + r) \
            * np.uint64(32) + k
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


def _lane_values(seed, wave):
    """[i][l] = D[(l>>4)*4+i][l&15] as uint64 (two's complement)."""
    d = ref_fold(seed, wave)
    lane = np.arange(64)
    return np.stack([d[(lane >> 4) * 4 + i, lane & 15] for i in range(4)]).view(np.uint64)


def ref_checksum(seed, wave, outer):
    """The recurrence as the plain loop over folds."""
    vals = _lane_values(seed, wave)
    c = np.zeros(64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for _ in range(outer):
            for i in range(4):
                c = c * np.uint64(G) + vals[i]
        return int(c.sum(dtype=np.uint64))


def ref_checksum_modular(seed, wave, outer):
    """The same value for a large `outer`, in Python integers mod 2^64."""
    vals = [[int(x) for x in row] for row in _lane_values(seed, wave)]
    s = sum(pow(G, 4 * j, 1 << 64) for j in range(outer)) & M64
    total = 0
    for lane in range(64):
        p = 0
        for i in range(4):
            p = (p * G + vals[i][lane]) & M64
        total += p
    return (total * s) & M64


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------

SYMBOLS = ("na_mfma_sweep_expected", "na_mfma_sweep_run", "na_mfma_sweep_verify", "na_mfma_sweep")


def test_library_exports_mfma_sweep_symbols():
    lib = ctypes.CDLL(_ensure_lib())
    for sym in SYMBOLS:
        assert hasattr(lib, sym), f"missing symbol {sym}"


@pytest.mark.parametrize(
    "seed,wave,corner,outer,checksum",
    [
        (0, 0, (251, 251, -25, -33), 1, 0xCC01126CE30E04E3),
        (7, 1, (-222, 112, 50, 78), 2, 0x002D3438BE4F31CA),
        (SEED, 5, (-154, -144, 120, 21), 3, 0x1B7411BE0EC33B24),
        (SEED, 4095, (63, 172, -39, -68), 3, 0x0C976162A9F81849),
    ],
)
def test_reference_known_answers(seed, wave, corner, outer, checksum):
    d = ref_fold(seed, wave)
    assert (int(d[0, 0]), int(d[0, 15]), int(d[15, 0]), int(d[15, 15])) == corner
    assert ref_checksum(seed, wave, outer) == checksum, f"{ref_checksum(seed, wave, outer):#x}"


def test_reference_values_and_bounds():
    a, b = ref_fragments(SEED, 3)
    assert set(np.unique(a)) == set(range(-3, 4)) and set(np.unique(b)) == set(range(-2, 3))
    # the fold is (sum A)(sum B), every element within 32 * 24 * 16
    d = ref_fold(SEED, 3)
    assert np.array_equal(d, a.sum(0) @ b.sum(0).T)
    assert np.abs(d).max() <= 12288
    # the two forms of the reference agree where both are affordable
    assert ref_checksum(SEED, 3, 3) == ref_checksum_modular(SEED, 3, 3)
    # waves and seeds get different data
    assert ref_checksum(SEED, 3, 1) != ref_checksum(SEED, 4, 1)
    assert ref_checksum(SEED, 3, 1) != ref_checksum(SEED + 1, 3, 1)


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


@pytest.mark.parametrize("seed", [0, 7, SEED])
@pytest.mark.parametrize("wave", [0, 1, 5, 4095])
def test_expected_checksum_matches_reference(cpu_agent, seed, wave):
    for outer in (1, 2, 3):
        assert cpu_agent.mfma_sweep_expected(wave, outer, seed) == ref_checksum(seed, wave, outer)
    assert cpu_agent.mfma_sweep_expected(wave, 1000, seed) == ref_checksum_modular(
        seed, wave, 1000)


def test_expected_checksum_argument_errors(cpu_agent):
    out = ctypes.c_uint64(0)
    lib = cpu_agent.lib
    u64 = ctypes.c_ulonglong
    assert lib.na_mfma_sweep_expected(u64(1), u64(0), 0, ctypes.byref(out)) == nodeagent.NA_ERR_ARG
    assert lib.na_mfma_sweep_expected(u64(1), u64(0), 1, None) == nodeagent.NA_ERR_ARG


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
    recs = _records(24, 2)
    rc, res = cpu_agent.mfma_sweep_verify(recs, 2)
    assert rc == nodeagent.NA_OK and res.ok
    assert (res.waves, res.bad_waves, res.units_seen, res.bad_units) == (24, 0, 6, 0)
    assert res.first_bad_wave == nodeagent.NO_BAD_WAVE and res.bad_simds == []
    # median of (2_100_000 + i) / 100_000 * 100 MHz over i = 0..23
    assert res.clock_mhz == pytest.approx(2100.012, abs=1e-6)
    # the same records do not verify under another fold count or seed
    assert cpu_agent.mfma_sweep_verify(recs, 3)[0] == nodeagent.NA_ERR_VERIFY
    assert cpu_agent.mfma_sweep_verify(recs, 2, SEED + 1)[1].bad_waves == 24


@pytest.mark.parametrize("wave,bit", [(0, 0), (13, 63), (23, 31)])
def test_verify_one_flipped_bit(cpu_agent, wave, bit):
    recs = _records(24, 2)
    recs[wave].checksum ^= 1 << bit
    rc, res = cpu_agent.mfma_sweep_verify(recs, 2)
    assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
    assert (res.bad_waves, res.bad_units, res.first_bad_wave) == (1, 1, wave)
    assert res.bad_simds == [_unit_of(wave)]
    assert res.units_seen == 6
    err = cpu_agent._err()
    assert nodeagent.mfma_unit_name(_unit_of(wave)) in err
    assert f"1 of 24 waves wrong on 1 CU(s), first wave {wave} " in err


def test_verify_two_records_of_one_unit(cpu_agent):
    recs = _records(24, 1)
    recs[9].checksum ^= 2
    recs[11].checksum ^= 1 << 40
    rc, res = cpu_agent.mfma_sweep_verify(recs, 1)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_waves, res.bad_units, res.first_bad_wave) == (2, 1, 9)
    assert res.bad_simds == [_unit_of(9), _unit_of(11)]
    # and two units when the second bad wave is another workgroup's
    recs[20].checksum ^= 1
    rc, res = cpu_agent.mfma_sweep_verify(recs, 1)
    assert (res.bad_waves, res.bad_units) == (3, 2)


def test_verify_record_in_the_wrong_place_is_bad(cpu_agent):
    recs = _records(8, 1)
    recs[5].wave = 6
    rc, res = cpu_agent.mfma_sweep_verify(recs, 1)
    assert rc == nodeagent.NA_ERR_VERIFY and (res.bad_waves, res.first_bad_wave) == (1, 5)


def test_verify_lists_a_bounded_number_of_units(cpu_agent):
    n = 4 * (nodeagent.MFMA_SWEEP_MAX_LISTED + 2)
    recs = _records(n, 1)
    for i in range(n):
        recs[i].checksum ^= 1
    rc, res = cpu_agent.mfma_sweep_verify(recs, 1)
    assert (res.bad_waves, res.bad_units) == (n, n // 4)
    assert res.bad_simds == [_unit_of(i) for i in range(nodeagent.MFMA_SWEEP_MAX_LISTED)]
    assert res.describe().endswith(", ...")


def test_run_argument_errors_before_any_hip_call(cpu_agent):
    lib = cpu_agent.lib
    recs = (nodeagent.MfmaRecord * 8)()
    ms = ctypes.c_double(0)
    seed = ctypes.c_ulonglong(SEED)

    def run(dtype, workgroups, outer, out, n_out):
        return lib.na_mfma_sweep_run(0, dtype, workgroups, outer, seed, out,
                                     ctypes.c_longlong(n_out), ctypes.byref(ms))

    for args in [(2, 2, 1, recs, 8), (-1, 2, 1, recs, 8), (0, 0, 1, recs, 8), (0, -3, 1, recs, 8),
                 (0, 2, 0, recs, 8), (1, 2, -1, recs, 8), (0, 2, 1, None, 8), (0, 2, 1, recs, 7),
                 (0, 3, 1, recs, 8)]:
        assert run(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_mfma_sweep_run" in cpu_agent._err()
    with pytest.raises(nodeagent.NodeAgentError):
        cpu_agent.mfma_sweep_run(0, "fp16")


# -- check() against a Python stand-in library --------------------------------

SICK_CU = (2, 1, 0, 5)


class FakeLib(MemtestFakeLib):
    """The memtest stand-in plus na_mfma_sweep. ``sweep``: {dev: "sick" |
    "slow"}; default clean. A sick GPU has one CU whose four SIMDs all
    compute wrong, in both dtypes."""

    def __init__(self, ngpu=1, sweep=None):
        super().__init__(ngpu=ngpu)
        self.sweep_calls = []
        sweep = sweep or {}

        def na_mfma_sweep(dev, dtype, workgroups, outer, seed, res, tflops):
            self.sweep_calls.append((dev, dtype, workgroups, outer, seed.value))
            kind = sweep.get(dev, "ok")
            r = res._obj
            r.waves, r.units_seen, r.clock_mhz = 4096, 256, 2251.26
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            tflops._obj.value = (0.5 if kind == "slow" else 2104.46) * (1 if dtype == 0 else 1.01)
            if kind != "sick":
                return 0
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 16, 1, 404, 4
            for simd in range(4):
                r.bad_list[simd][:] = SICK_CU + (simd,)
            r.first_bad_unit[:] = SICK_CU + (0,)
            return nodeagent.NA_ERR_VERIFY

        self.na_mfma_sweep = na_mfma_sweep


def _agent(monkeypatch, **kw):
    fake = FakeLib(**kw)
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fake)
    return nodeagent.NodeAgent(), fake


def _sweep_fields(g):
    return (g.mfma_sweep_tflops, g.mfma_sweep_fp8_tflops, g.mfma_sweep_clock_mhz,
            g.mfma_sweep_units_seen, g.mfma_sweep_bad_waves)


def test_check_default_never_runs_sweep(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check()
    assert fake.sweep_calls == []
    assert report.healthy, report.problems
    assert _sweep_fields(report.gpus[0]) == (0.0, 0.0, 0.0, 0, 0)
    assert _sweep_fields(nodeagent.GPUReport(index=0)) == (0.0, 0.0, 0.0, 0, 0)
    # the stand-in of the memtest tests has no sweep function at all
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: MemtestFakeLib())
    assert nodeagent.NodeAgent().check(memtest_bytes=1024).healthy


def test_check_clean_sweep_populates_fields(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check(mfma_sweep=True)
    assert fake.sweep_calls == [(0, 0, 0, 0, SEED), (0, 1, 0, 0, SEED)]
    g = report.gpus[0]
    assert report.healthy and g.healthy, report.problems
    assert _sweep_fields(g) == (2104.5, 2125.5, 2251.3, 256, 0)
    assert nodeagent.node_condition_from_report(report)["status"] == "True"


def test_check_units_seen_below_cus_is_reported_not_a_problem(monkeypatch):
    agent, fake = _agent(monkeypatch)
    real = fake.na_mfma_sweep

    def fewer(dev, dtype, workgroups, outer, seed, res, tflops):
        rc = real(dev, dtype, workgroups, outer, seed, res, tflops)
        res._obj.units_seen = 255
        return rc

    fake.na_mfma_sweep = fewer
    report = agent.check(mfma_sweep=True)
    assert report.gpus[0].mfma_sweep_units_seen == 255 < report.gpus[0].cus
    assert report.healthy, report.problems


def test_check_eight_gpus_one_sick_cu(monkeypatch):
    agent, fake = _agent(monkeypatch, ngpu=8, sweep={3: "sick"})
    report = agent.check(expect_gpus=8, mfma_sweep=True)
    assert [c[:2] for c in fake.sweep_calls] == [(d, t) for d in range(8) for t in (0, 1)]
    want = [
        f"gpu3: MFMA sweep {dtype}: 16 of 4096 waves wrong on 1 CU(s): "
        "xcc2.se1.sh0.cu5 simd 0,1,2,3"
        for dtype in ("bf16", "fp8")
    ]
    assert report.problems == want
    assert not report.healthy
    assert [g.healthy for g in report.gpus] == [i != 3 for i in range(8)]
    assert [g.mfma_sweep_bad_waves for g in report.gpus] == [32 if i == 3 else 0 for i in range(8)]
    assert nodeagent.node_condition_from_report(report) == {
        "type": karpv1.AMD_GPU_HEALTHY_CONDITION_TYPE,
        "status": "False",
        "reason": "GPUUnhealthy",
        "message": "; ".join(want),
    }


def test_check_low_tflops_flags_a_problem(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_MFMA_SWEEP_TFLOPS", 1400.0)
    agent, _ = _agent(monkeypatch, sweep={0: "slow"})
    report = agent.check(mfma_sweep=True)
    assert report.gpus[0].problems == ["MFMA sweep bf16 0.5 TFLOP/s below floor 1400.0"]
    assert not report.healthy
    # a healthy rate passes the same floor
    agent, _ = _agent(monkeypatch)
    assert agent.check(mfma_sweep=True).healthy


def test_cli_flag_reaches_check(monkeypatch, capsys):
    _, fake = _agent(monkeypatch)
    assert nodeagent.main(["--mfma-sweep"]) == 0
    assert [c[:2] for c in fake.sweep_calls] == [(0, 0), (0, 1)]
    assert json.loads(capsys.readouterr().out)["gpus"][0]["mfma_sweep_units_seen"] == 256
    _, fake = _agent(monkeypatch)
    assert nodeagent.main([]) == 0
    assert fake.sweep_calls == []
    capsys.readouterr()


def test_chart_passes_mfma_sweep_only_when_true():
    import yaml

    chart = os.path.join(ROOT, "charts", "gpu-provisioner-amd")
    with open(os.path.join(chart, "values.yaml")) as f:
        values = yaml.safe_load(f)
    assert values["nodeAgent"]["mfmaSweep"] is False
    with open(os.path.join(chart, "templates", "amd-gpu-node-stack.yaml")) as f:
        text = f.read()
    start = text.index("{{- if .Values.nodeAgent.mfmaSweep }}")
    end = text.index("{{- end }}", start)
    assert "--mfma-sweep \\" in text[start:end]
    assert text.count("--mfma-sweep") == 1  # nowhere outside the guard


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


_runs = {}


def _run(agent, dtype, workgroups, outer, seed=SEED):
    """One launch per distinct shape, shared by the tests; read-only."""
    key = (dtype, workgroups, outer, seed)
    if key not in _runs:
        torch.cuda.synchronize()
        _runs[key] = agent.mfma_sweep_run(0, dtype, workgroups, outer, seed)[0]
    return _runs[key]


_sweeps = {}


def _default_sweep(agent, dtype):
    if dtype not in _sweeps:
        torch.cuda.synchronize()
        _sweeps[dtype] = agent.mfma_sweep(0, dtype)
    return _sweeps[dtype]


# (1, 1): one workgroup, one fold; (3, 2): wave indexing across workgroups
# and the chaining of folds (the loop is pipelined by one fold, so outer = 1
# and outer = 2 leave it by different paths)
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,workgroups,outer", [("bf16", 1, 1), ("bf16", 3, 2), ("fp8", 3, 2),
                                                    ("fp8", 1, 1), ("bf16", 2, 3)])
def test_gpu_record_checksums_match_reference(agent, dtype, workgroups, outer):
    recs = _run(agent, dtype, workgroups, outer)
    assert len(recs) == 4 * workgroups
    for w, r in enumerate(recs):
        assert r.checksum == ref_checksum(SEED, w, outer), f"{dtype} wave {w}: {r.checksum:#x}"


@pytest.mark.gpu
def test_gpu_dtypes_agree_and_seed_matters(agent):
    bf16 = [r.checksum for r in _run(agent, "bf16", 3, 2)]
    fp8 = [r.checksum for r in _run(agent, "fp8", 3, 2)]
    other = [r.checksum for r in _run(agent, "bf16", 3, 2, seed=7)]
    assert bf16 == fp8
    assert all(a != b for a, b in zip(bf16, other))
    assert other == [ref_checksum(7, w, 2) for w in range(12)]


@pytest.mark.gpu
def test_gpu_record_sanity(agent):
    recs = _run(agent, "bf16", 8, 2)
    assert [r.wave for r in recs] == list(range(32))
    for r in recs:
        assert r.xcc < 8 and r.se < 4 and r.sh < 2 and r.cu < 16 and r.simd < 4
        assert r.cycles > 0 and r.realtime > 0
    for wg in range(8):
        waves = recs[4 * wg: 4 * wg + 4]
        assert len({(r.xcc, r.se, r.sh, r.cu) for r in waves}) == 1, f"workgroup {wg}"
        assert sorted(r.simd for r in waves) == [0, 1, 2, 3], f"workgroup {wg}"


@pytest.mark.gpu
def test_gpu_localisation_on_own_records(agent):
    src = _run(agent, "bf16", 8, 2)
    rc, res = agent.mfma_sweep_verify(src, 2)
    assert rc == nodeagent.NA_OK and res.ok and res.waves == 32
    assert 1 <= res.units_seen <= 8
    recs = (nodeagent.MfmaRecord * len(src))()
    ctypes.memmove(recs, src, ctypes.sizeof(src))  # the shared run stays as it came back
    recs[21].checksum ^= 1 << 17
    rc, res = agent.mfma_sweep_verify(recs, 2)
    assert rc == nodeagent.NA_ERR_VERIFY
    unit = (recs[21].xcc, recs[21].se, recs[21].sh, recs[21].cu, recs[21].simd)
    assert (res.bad_waves, res.bad_units, res.first_bad_wave) == (1, 1, 21)
    assert res.bad_simds == [unit]
    assert nodeagent.mfma_unit_name(unit) in agent._err()


def _sanity_bound_tflops(agent):
    """1024 FLOP/clk/SIMD (one 16384-FLOP MFMA per 16 cycles) x 4 SIMDs x CUs
    x the device's maximum clock, +2 %."""
    name = ctypes.create_string_buffer(256)
    arch = ctypes.create_string_buffer(256)
    hbm, cus, khz = ctypes.c_longlong(0), ctypes.c_int(0), ctypes.c_int(0)
    assert agent.lib.na_device_info(0, name, 256, arch, 256, ctypes.byref(hbm),
                                    ctypes.byref(cus), ctypes.byref(khz)) == 0
    return cus.value, 1024 * 4 * cus.value * khz.value * 1e3 * 1.02 / 1e12


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_gpu_default_sweep(agent, dtype):
    res = _default_sweep(agent, dtype)
    cus, bound = _sanity_bound_tflops(agent)
    print(f"mfma_sweep {dtype}: {res.tflops:.1f} TFLOP/s (bound {bound:.1f}), "
          f"{res.clock_mhz:.0f} MHz, {res.units_seen} of {cus} CUs, {res.waves} waves")
    assert res.ok, res.describe()
    assert res.waves == 16 * cus and res.bad_waves == 0 and res.bad_simds == []
    assert 1 <= res.units_seen <= cus
    assert 0 < res.tflops < bound
    assert res.clock_mhz > 0


@pytest.mark.gpu
def test_gpu_check_with_sweep(agent):
    torch.cuda.synchronize()
    report = agent.check(bw_bytes=1 << 28, mfma_sweep=True)
    g0 = report.gpus[0]
    assert g0.healthy, g0.problems
    assert g0.mfma_sweep_tflops > 0 and g0.mfma_sweep_fp8_tflops > 0
    assert g0.mfma_sweep_clock_mhz > 0
    assert 1 <= g0.mfma_sweep_units_seen <= g0.cus
    assert g0.mfma_sweep_bad_waves == 0


@pytest.mark.gpu
def test_gpu_cli_mfma_sweep():
    _ensure_lib()
    proc = subprocess.run(
        [sys.executable, "-m", "gpu_provisioner_amd.nodeagent", "--json",
         "--bw-bytes", "268435456", "--mfma-sweep"],
        capture_output=True,
        text=True,
        cwd=ROOT,
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    report = json.loads(proc.stdout)
    assert report["healthy"] is True
    g0 = report["gpus"][0]
    assert g0["mfma_sweep_bad_waves"] == 0
    assert g0["mfma_sweep_tflops"] > 0 and g0["mfma_sweep_fp8_tflops"] > 0
    assert 1 <= g0["mfma_sweep_units_seen"] <= g0["cus"]
