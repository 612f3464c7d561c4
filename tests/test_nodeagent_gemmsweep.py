"""Chip-wide GEMM sweep of the node agent (nodeagent/gemmsweep.h): C = reps *
A * B^T on hashed small-integer operands, from device memory through L2 and a
swizzled, double-buffered LDS into the bf16 or fp8 MFMA, one 256 x 256 tile
per workgroup and one weighted checksum per wave.

The reference is the numpy copy of the specification below: operands from the
hash, C by a plain matrix product, every wave's checksum as the direct sum of
p_i * q_j * C[i][j]. It shares nothing with the host code's U/V dot products.
The GPU tests change one operand element of their own tensor to see detection:
a data mismatch; nothing on the GPU is provoked.
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
from tests.test_nodeagent_mfmasweep import _mix64

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
U64 = np.uint64
SEED = getattr(nodeagent, "DEFAULT_GEMM_SWEEP_SEED", 0)
BK = {"bf16": 64, "fp8": 128}
# (M, N, K / BK): one tile without pipelining; both LDS buffers; buffer reuse;
# tile order, row against column; 6 tiles and an odd step count; 9 tiles, no
# multiple of the 8 XCDs; 12 tiles, wrapping them
SHAPES = [(256, 256, 1), (256, 256, 2), (256, 256, 3), (512, 256, 1), (256, 512, 1),
          (768, 512, 5), (768, 768, 2), (1024, 768, 2)]
CASES = [(s, 1) for s in SHAPES] + [((256, 256, 3), 3), ((768, 512, 5), 3)]
# E4M3 bytes of -3..3: sign, exponent (bias 7), three mantissa bits
E4M3 = {0x00: 0, 0x38: 1, 0x40: 2, 0x44: 3, 0xB8: -1, 0xC0: -2, 0xC4: -3}


def _ensure_lib():
    import __graft_entry__ as g

    if not os.path.exists(g.LIB_PATH):
        g.build()
    return g.LIB_PATH


@functools.lru_cache(maxsize=None)
def ref(seed, m, n, k, reps):
    """(A, B, C, checksums) of the specification: the direct sum per wave."""
    with np.errstate(over="ignore"):
        def hashed(first, count):
            return _mix64(U64((seed * G + first) & M64) + np.arange(count, dtype=U64))

        a = ((hashed(0, m * k) >> U64(40)) % U64(7)).astype(np.int64).reshape(m, k) - 3
        b = ((hashed(m * k, n * k) >> U64(40)) % U64(5)).astype(np.int64).reshape(n, k) - 2
        p = hashed(m * k + n * k, m) | U64(1)
        q = hashed(m * k + n * k + m, n) | U64(1)
        # small integers: the float64 product is exact
        c = reps * (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)
        weighted = p[:, None] * q[None, :] * c.astype(U64)
        sums = weighted.reshape(m // 256, 2, 128, n // 256, 2, 128).sum(axis=(2, 5), dtype=U64)
    # [ti][wr][tj][wc] -> record 4 * (ti * (n / 256) + tj) + 2 * wr + wc
    return a, b, c, [int(x) for x in sums.transpose(0, 2, 1, 3).reshape(-1)]


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("shape,reps", CASES)
def test_expected_matches_direct_sum(cpu_agent, shape, reps, dtype):
    m, n, k = shape[0], shape[1], shape[2] * BK[dtype]
    assert cpu_agent.gemm_sweep_expected(m, n, k, reps, SEED) == ref(SEED, m, n, k, reps)[3]
    if shape == SHAPES[4]:  # and a seed past 2^40, whose high half matters
        big = (1 << 40) + 9
        got = cpu_agent.gemm_sweep_expected(m, n, k, reps, big)
        assert got == ref(big, m, n, k, reps)[3] and len(set(got)) == 8
        assert got != cpu_agent.gemm_sweep_expected(m, n, k, reps, big & 0xFFFFFFFF)


@pytest.mark.parametrize("m,n,k,reps", [
    (255, 256, 64, 1), (256, 384, 64, 1), (0, 256, 64, 1), (256, 256, 96, 1), (256, 256, 0, 1),
    (256, 256, 64, 0), (256, 256, 8192, 342), (256, 256, 1 << 22, 1)])
def test_shape_errors_before_any_hip_call(cpu_agent, m, n, k, reps):
    lib, tiles = cpu_agent.lib, max(m // 256 * (n // 256), 1)
    out, recs = (ctypes.c_uint64 * (4 * tiles))(), (nodeagent.MfmaRecord * (4 * tiles))()
    res, ptr = nodeagent._MfmaSweepResultC(), 1 << 40  # the pointer is never followed
    assert lib.na_gemm_sweep_expected(SEED, m, n, k, reps, out, len(out)) == nodeagent.NA_ERR_ARG
    assert "na_gemm_sweep_expected" in cpu_agent._err()
    assert lib.na_gemm_sweep_run(0, 0, ptr, ptr, None, m, n, k, reps, SEED, recs, len(recs),
                                 None) == nodeagent.NA_ERR_ARG
    assert lib.na_gemm_sweep_verify(recs, len(recs), m, n, k, reps, SEED,
                                    ctypes.byref(res)) == nodeagent.NA_ERR_ARG
    assert lib.na_gemm_sweep(0, 0, m or 255, n, k or 8, reps or -1, SEED, ctypes.byref(res),
                             None) == nodeagent.NA_ERR_ARG
    if reps == 1:  # the fill takes no reps
        assert lib.na_gemm_sweep_fill(0, 0, ptr, ptr, m, n, k, SEED) == nodeagent.NA_ERR_ARG


def test_other_argument_errors_before_any_hip_call(cpu_agent):
    lib, ptr = cpu_agent.lib, 1 << 40
    out, recs, res = (ctypes.c_uint64 * 8)(), (nodeagent.MfmaRecord * 8)(), nodeagent._MfmaSweepResultC()
    bad = nodeagent.NA_ERR_ARG
    assert lib.na_gemm_sweep_expected(SEED, 256, 512, 64, 1, out, 7) == bad
    assert lib.na_gemm_sweep_expected(SEED, 256, 256, 64, 1, out, 8) == bad
    assert lib.na_gemm_sweep_expected(SEED, 256, 512, 64, 1, None, 8) == bad
    for a, b, dtype, k, n_out in [(None, ptr, 0, 64, 8), (ptr, None, 0, 64, 8), (ptr + 8, ptr, 0, 64, 8),
                                  (ptr, ptr, 2, 128, 8), (ptr, ptr, -1, 128, 8),
                                  (ptr, ptr, 1, 64, 8),  # fp8 needs a multiple of 128
                                  (ptr, ptr, 0, 64, 4), (ptr, ptr, 0, 64, 12)]:
        rc = lib.na_gemm_sweep_run(0, dtype, a, b, None, 256, 512, k, 1, SEED, recs, n_out, None)
        assert rc == bad and "na_gemm_sweep_run" in cpu_agent._err(), (a, b, dtype, k, n_out)
    assert lib.na_gemm_sweep_run(0, 0, ptr, ptr, None, 256, 512, 64, 1, SEED, None, 8, None) == bad
    assert lib.na_gemm_sweep_fill(0, 0, None, ptr, 256, 512, 64, SEED) == bad
    assert lib.na_gemm_sweep_fill(0, 3, ptr, ptr, 256, 512, 128, SEED) == bad
    assert lib.na_gemm_sweep_verify(recs, 4, 256, 512, 64, 1, SEED, ctypes.byref(res)) == bad
    assert lib.na_gemm_sweep_verify(None, 8, 256, 512, 64, 1, SEED, ctypes.byref(res)) == bad
    assert lib.na_gemm_sweep_verify(recs, 8, 256, 512, 64, 1, SEED, None) == bad
    assert lib.na_gemm_sweep(0, 2, 0, 0, 0, 0, SEED, ctypes.byref(res), None) == bad
    assert lib.na_gemm_sweep(0, 0, 0, 0, 0, 0, SEED, None, None) == bad


@pytest.mark.parametrize("wave", [0, 13, 23])
def test_verify_names_the_unit_tile_and_sub_tile_of_one_wrong_record(cpu_agent, wave):
    m, n, k, reps = 768, 512, 128, 2
    want = ref(SEED, m, n, k, reps)[3]
    recs = (nodeagent.MfmaRecord * len(want))()
    for i, r in enumerate(recs):
        r.checksum, r.wave, r.cycles, r.realtime = want[i], i, 21000, 1000
        r.xcc, r.se, r.sh, r.cu, r.simd = i // 4 % 8, i // 32 % 4, 0, i // 4 % 16, i % 4
    rc, res = cpu_agent.gemm_sweep_verify(recs, m, n, k, reps, SEED)
    assert rc == nodeagent.NA_OK and res.ok and res.sweep.waves == 24
    assert res.sweep.units_seen == 6 and res.sweep.clock_mhz == pytest.approx(2100.0)
    recs[wave].checksum ^= 1 << 17
    rc, res = cpu_agent.gemm_sweep_verify(recs, m, n, k, reps, SEED)
    assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
    assert (res.sweep.bad_waves, res.sweep.first_bad_wave) == (1, wave)
    r, t = recs[wave], wave // 4
    unit = f"xcc{r.xcc}.se{r.se}.sh0.cu{r.cu}.simd{wave % 4}"
    where = f"tile {t // 2},{t % 2} sub-tile {wave >> 1 & 1},{wave & 1}"
    assert f"first wave {wave} ({where}) on {unit}" in cpu_agent._err()
    assert f"{unit} computed tile ({t // 2},{t % 2}) sub-tile ({wave >> 1 & 1},{wave & 1})" \
        in res.describe()


class FakeLib(MfmaFakeLib):
    """The matrix-core sweep's stand-in plus na_gemm_sweep. ``gemm``: {dev:
    "sick" | "slow" | "noroom"}; default clean."""

    def __init__(self, ngpu=1, gemm=None):
        super().__init__(ngpu=ngpu)
        self.gemm_calls = []

        def na_gemm_sweep(dev, dtype, m, n, k, reps, seed, res, tflops):
            self.gemm_calls.append((dev, dtype, m, n, k, reps, seed))
            kind = (gemm or {}).get(dev, "ok")
            if kind == "noroom":
                self.error = b"na_gemm_sweep: the operands of 268435456 bytes do not fit: 1 bytes"
                return nodeagent.NA_ERR_ARG
            r = res._obj
            r.waves, r.units_seen, r.clock_mhz = 4096, 256, 1801.26
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            tflops._obj.value = 1.5 if kind == "slow" else 901.26
            if kind != "sick":
                return 0
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 1, 1, 4 * 37 + 2, 1
            r.bad_list[0][:] = r.first_bad_unit[:] = (5, 2, 1, 9, 3)
            return nodeagent.NA_ERR_VERIFY

        self.na_gemm_sweep = na_gemm_sweep


def test_flag_reaches_check_through_the_cli(monkeypatch, capsys):
    monkeypatch.setattr(nodeagent, "MIN_GEMM_SWEEP_TFLOPS", 600.0)
    fakes = []
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fakes[-1])
    fakes.append(FakeLib())
    assert nodeagent.main([]) == 0 and fakes[-1].gemm_calls == []
    capsys.readouterr()
    assert nodeagent.main(["--gemm-sweep"]) == 0
    assert fakes[-1].gemm_calls == [(0, 0, 0, 0, 0, 0, SEED)] and fakes[-1].sweep_calls == []
    g = json.loads(capsys.readouterr().out)["gpus"][0]
    assert [g[f"gemm_sweep_{f}"] for f in ("tflops", "clock_mhz", "units_seen", "bad_waves",
                                           "skipped")] == [901.3, 1801.3, 256, 0, ""]
    fakes.append(FakeLib(ngpu=2, gemm={1: "sick"}))
    report = nodeagent.NodeAgent().check(gemm_sweep=True)
    assert report.problems == [
        "gpu1: GEMM sweep: 1 of 4096 waves wrong on 1 CU(s): xcc5.se2.sh1.cu9 simd 3; first wave "
        "150 on xcc5.se2.sh1.cu9.simd3 computed tile (1,5) sub-tile (1,0)"]
    assert nodeagent.node_condition_from_report(report)["status"] == "False"
    fakes.append(FakeLib(gemm={0: "slow"}))
    assert nodeagent.NodeAgent().check(gemm_sweep=True).gpus[0].problems == [
        "GEMM sweep 1.5 TFLOP/s below floor 600.0"]
    fakes.append(FakeLib(gemm={0: "noroom"}))
    g = nodeagent.NodeAgent().check(gemm_sweep=True).gpus[0]
    assert g.healthy and "do not fit" in g.gemm_sweep_skipped and g.gemm_sweep_tflops == 0.0


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _operands(agent, dtype, m, n, k):
    kind = torch.bfloat16 if dtype == "bf16" else torch.uint8
    a = torch.empty((m, k), dtype=kind, device="cuda:0")
    b = torch.empty((n, k), dtype=kind, device="cuda:0")
    torch.cuda.synchronize()
    agent.gemm_sweep_fill(0, a.data_ptr(), b.data_ptr(), m, n, k, SEED, dtype)
    return a, b


def _values(x, dtype):
    if dtype == "bf16":
        return x.float().cpu().numpy().astype(np.int64)
    table = np.full(256, 99, dtype=np.int64)
    table[list(E4M3)] = list(E4M3.values())
    return table[x.cpu().numpy()]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("shape,reps", CASES)
def test_gpu_gemm(agent, shape, reps, dtype):
    m, n, k = shape[0], shape[1], shape[2] * BK[dtype]
    want_a, want_b, want_c, want_sums = ref(SEED, m, n, k, reps)
    a, b = _operands(agent, dtype, m, n, k)
    c = torch.full((m, n), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    recs, ms = agent.gemm_sweep_run(0, a.data_ptr(), b.data_ptr(), m, n, k, reps, SEED, dtype,
                                    c.data_ptr())
    print(f"{dtype} {m}x{n}x{k} reps {reps}: {ms:.3f} ms, SIMDs {[r.simd for r in recs]}")
    assert np.array_equal(_values(a, dtype), want_a) and np.array_equal(_values(b, dtype), want_b)
    assert np.array_equal(c.cpu().numpy().astype(np.int64), want_c)
    assert [r.checksum for r in recs] == want_sums
    assert [r.wave for r in recs] == list(range(len(want_sums)))
    rc, res = agent.gemm_sweep_verify(recs, m, n, k, reps, SEED, dtype)
    assert rc == nodeagent.NA_OK and res.sweep.bad_waves == 0, agent._err()
    for t in range(len(recs) // 4):
        four = recs[4 * t:4 * t + 4]
        assert len({(r.xcc, r.se, r.sh, r.cu) for r in four}) == 1
        assert sorted(r.simd for r in four) == [0, 1, 2, 3]
        assert all(r.cycles > 0 and r.realtime > 0 for r in four)
    again, _ms = agent.gemm_sweep_run(0, a.data_ptr(), b.data_ptr(), m, n, k, reps, SEED, dtype)
    assert [r.checksum for r in again] == want_sums


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_gpu_one_changed_element_is_seen_by_the_waves_that_read_its_row(agent, dtype):
    m, n, k, row, col = 768, 512, 2 * BK[dtype], 400, BK[dtype] + 17
    a, b = _operands(agent, dtype, m, n, k)
    was = int(_values(a[row:row + 1, col:col + 1], dtype)[0, 0])
    now = 1 if was != 1 else 2  # another small integer, exact in both formats
    a[row, col] = now if dtype == "bf16" else next(c for c, v in E4M3.items() if v == now)
    torch.cuda.synchronize()
    recs, _ms = agent.gemm_sweep_run(0, a.data_ptr(), b.data_ptr(), m, n, k, 1, SEED, dtype)
    rc, res = agent.gemm_sweep_verify(recs, m, n, k, 1, SEED, dtype)
    want = ref(SEED, m, n, k, 1)[3]
    bad = [i for i, r in enumerate(recs) if r.checksum != want[i]]
    # row 400: tile row 1, its lower 128 rows (wr 1), in both tile columns and both wc
    assert bad == [4 * (1 * 2 + tj) + 2 * 1 + wc for tj in range(2) for wc in range(2)]
    assert rc == nodeagent.NA_ERR_VERIFY and res.sweep.bad_waves == 2 * (n // 256)
    assert res.sweep.first_bad_wave == bad[0] and "tile 1,0 sub-tile 1,0" in agent._err()


@pytest.mark.gpu
def test_gpu_default_sweep(agent):
    torch.cuda.synchronize()
    res = agent.gemm_sweep(0)
    _, _, _, cus = agent.device_info(0)
    print(f"gemm_sweep: {res.tflops:.1f} TFLOP/s at {res.sweep.clock_mhz:.0f} MHz, "
          f"{res.sweep.units_seen} of {cus} CUs, {res.sweep.waves} waves")
    assert res.ok, res.describe()
    assert res.sweep.waves == 4 * 32 * 32 and res.sweep.units_seen == cus
    assert res.tflops >= nodeagent.MIN_GEMM_SWEEP_TFLOPS > 0


@pytest.mark.gpu
def test_gpu_check_with_sweep(agent):
    torch.cuda.synchronize()
    report = agent.check(bw_bytes=1 << 28, gemm_sweep=True)
    g0 = report.gpus[0]
    assert g0.healthy, g0.problems
    assert g0.gemm_sweep_tflops >= nodeagent.MIN_GEMM_SWEEP_TFLOPS
    assert g0.gemm_sweep_clock_mhz > 0 and g0.gemm_sweep_units_seen == g0.cus
    assert g0.gemm_sweep_bad_waves == 0 and g0.gemm_sweep_skipped == ""
