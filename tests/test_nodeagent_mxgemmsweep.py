"""Chip-wide block-scaled MX GEMM sweep of the node agent
(nodeagent/mxgemmsweep.h): C = reps * sum_k 2^ea a * 2^eb b on hashed operands in
MXFP8 or MXFP4 and hashed E8M0 scales, both from device memory through L2 and
LDS into v_mfma_scale_f32_16x16x128_f8f6f4.

The reference is the numpy copy of the specification below: operands and scale
exponents from the hash, C by a plain matrix product of the scaled operands,
every wave's checksum as the direct sum of p_i * q_j * C[i][j]. The GPU tests
change one scale byte of their own tensor to see detection: a data mismatch;
nothing on the GPU is provoked.
"""
import ctypes
import functools
import json

import numpy as np
import pytest

# torch first, before any test loads the agent library: see the note at the
# top of test_nodeagent_memtest.py (one HIP runtime per process — torch's).
try:
    import torch
except ImportError:  # CPU-only environment: the GPU tests cannot run there
    torch = None

from gpu_provisioner_amd import nodeagent
from tests.test_nodeagent_gemmsweep import FakeLib as GemmFakeLib
from tests.test_nodeagent_gemmsweep import _ensure_lib
from tests.test_nodeagent_mfmasweep import _mix64

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
U64 = np.uint64
SEED = getattr(nodeagent, "DEFAULT_MXGEMM_SWEEP_SEED", 0)
FORMATS = ["fp8", "fp4"]
BK = {"fp8": 128, "fp4": 256}
# (M, N, K / BK): one tile without pipelining; both LDS stages; stage reuse;
# tile order, row against column; 6 tiles and an odd step count; 12 tiles,
# wrapping the 8 XCDs
SHAPES = [(256, 256, 1), (256, 256, 2), (256, 256, 3), (512, 256, 1), (256, 512, 1),
          (768, 512, 5), (1024, 768, 2)]
CASES = [(s, 1) for s in SHAPES] + [((256, 256, 3), 3), ((768, 512, 5), 3)]
# codes of -3..3: E4M3 bytes (bias 7, three mantissa bits), E2M1 nibbles (bias 1, one)
CODES = {"fp8": {0x00: 0, 0x38: 1, 0x40: 2, 0x44: 3, 0xB8: -1, 0xC0: -2, 0xC4: -3},
         "fp4": {0x0: 0, 0x2: 1, 0x4: 2, 0x5: 3, 0xA: -1, 0xC: -2, 0xD: -3}}


@functools.lru_cache(maxsize=None)
def ref(seed, m, n, k, reps):
    """(a, b, ea, eb, C, checksums) of the specification: the direct sum per wave."""
    s = k // 32
    with np.errstate(over="ignore"):
        def hashed(first, count):
            return _mix64(U64((seed * G + first) & M64) + np.arange(count, dtype=U64))

        def drawn(first, rows, cols, mod):
            return ((hashed(first, rows * cols) >> U64(40)) % U64(mod)).astype(np.int64).reshape(
                rows, cols)

        a, b = drawn(0, m, k, 7) - 3, drawn(m * k, n, k, 5) - 2
        ea = drawn(m * k + n * k, m, s, 2)
        eb = drawn(m * k + n * k + m * s, n, s, 2)
        p = hashed(m * k + n * k + m * s + n * s, m) | U64(1)
        q = hashed(m * k + n * k + m * s + n * s + m, n) | U64(1)
        scaled_a = (a << np.repeat(ea, 32, axis=1)).astype(np.float64)
        scaled_b = (b << np.repeat(eb, 32, axis=1)).astype(np.float64)
        c = reps * (scaled_a @ scaled_b.T).astype(np.int64)  # small integers: exact in float64
        weighted = p[:, None] * q[None, :] * c.astype(U64)
        sums = weighted.reshape(m // 256, 2, 128, n // 256, 2, 128).sum(axis=(2, 5), dtype=U64)
    # [ti][wr][tj][wc] -> record 4 * (ti * (n / 256) + tj) + 2 * wr + wc
    return a, b, ea, eb, c, [int(x) for x in sums.transpose(0, 2, 1, 3).reshape(-1)]


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape,reps", CASES)
def test_expected_matches_direct_sum(cpu_agent, shape, reps, fmt):
    m, n, k = shape[0], shape[1], shape[2] * BK[fmt]
    assert nodeagent.MXGEMM_SWEEP_BK == BK and list(nodeagent.MXGEMM_SWEEP_FORMATS) == FORMATS
    assert cpu_agent.mxgemm_sweep_expected(m, n, k, reps, SEED) == ref(SEED, m, n, k, reps)[5]
    if shape == SHAPES[0]:
        # a block mix-up must not hide: some row of A and some of B carries both
        # scale values within one 128-element group (the four blocks of an MFMA)
        for e in ref(SEED, m, n, k, reps)[2:4]:
            groups = e.reshape(e.shape[0], -1, 4)
            assert (groups.min(axis=2) != groups.max(axis=2)).any()
        big = (1 << 40) + 9  # and a seed whose high half matters
        assert cpu_agent.mxgemm_sweep_expected(m, n, k, reps, big) == ref(big, m, n, k, reps)[5]


@pytest.mark.parametrize("fmt,m,n,k,reps", [
    (0, 255, 256, 128, 1), (0, 256, 384, 128, 1), (0, 0, 256, 128, 1), (0, 256, 256, 64, 1),
    (0, 256, 256, 0, 1), (0, 256, 256, 128, 0), (0, 256, 256, 8192, 86), (0, 256, 256, 1 << 22, 1),
    (4, 256, 256, 128, 1),  # fp4 needs a multiple of 256
    (1, 256, 256, 256, 1), (2, 256, 256, 256, 1), (-1, 256, 256, 256, 1)])  # no such format
def test_shape_exactness_and_format_errors_before_any_hip_call(cpu_agent, fmt, m, n, k, reps):
    lib, tiles, bad = cpu_agent.lib, max(m // 256 * (n // 256), 1), nodeagent.NA_ERR_ARG
    out, recs = (ctypes.c_uint64 * (4 * tiles))(), (nodeagent.MfmaRecord * (4 * tiles))()
    res, ptr = nodeagent._MfmaSweepResultC(), 1 << 40  # the pointer is never followed
    assert lib.na_mxgemm_sweep_run(0, fmt, ptr, ptr, ptr, ptr, None, m, n, k, reps, SEED, recs,
                                   len(recs), None) == bad
    assert "na_mxgemm_sweep_run" in cpu_agent._err()
    assert lib.na_mxgemm_sweep(0, fmt, m or 255, n, k or 8, reps or -1, SEED, ctypes.byref(res),
                               None) == bad
    if reps == 1:  # the fill takes no reps
        assert lib.na_mxgemm_sweep_fill(0, fmt, ptr, ptr, ptr, ptr, m, n, k, SEED) == bad
    if k % 128 or k == 0 or reps != 1 or k > 8192 or m % 256 or n % 256 or m == 0:
        # what no format allows: expected and verify take no format
        assert lib.na_mxgemm_sweep_expected(SEED, m, n, k, reps, out, len(out)) == bad
        assert lib.na_mxgemm_sweep_verify(recs, len(recs), m, n, k, reps, SEED,
                                          ctypes.byref(res)) == bad


def test_pointer_and_name_errors_before_any_hip_call_and_the_cap_is_allowed(cpu_agent):
    recs, ptr = (nodeagent.MfmaRecord * 4)(), 1 << 40
    for a, sb in [(None, ptr), (ptr + 8, ptr), (ptr, None), (ptr, ptr + 4)]:
        assert cpu_agent.lib.na_mxgemm_sweep_run(0, 0, a, ptr, ptr, sb, None, 256, 256, 128, 1,
                                                 SEED, recs, 4, None) == nodeagent.NA_ERR_ARG
    assert cpu_agent.mxgemm_sweep_expected(256, 256, 8192, 85, SEED)  # 24 * 85 * 8192 < 2^24
    with pytest.raises(nodeagent.NodeAgentError, match="'fp6' is not one of fp8, fp4"):
        cpu_agent.mxgemm_sweep(0, "fp6")


@pytest.mark.parametrize("wave", [0, 13, 23])
def test_verify_names_the_unit_tile_and_sub_tile_of_one_wrong_record(cpu_agent, wave):
    m, n, k, reps = 768, 512, 256, 2
    want = ref(SEED, m, n, k, reps)[5]
    recs = (nodeagent.MfmaRecord * len(want))()
    for i, r in enumerate(recs):
        r.checksum, r.wave, r.cycles, r.realtime = want[i], i, 21000, 1000
        r.xcc, r.se, r.sh, r.cu, r.simd = i // 4 % 8, i // 32 % 4, 0, i // 4 % 16, i % 4
    rc, res = cpu_agent.mxgemm_sweep_verify(recs, m, n, k, reps, SEED)
    assert rc == nodeagent.NA_OK and res.ok and res.sweep.waves == 24 and res.sweep.units_seen == 6
    recs[wave].checksum ^= 1 << 17
    rc, res = cpu_agent.mxgemm_sweep_verify(recs, m, n, k, reps, SEED)
    assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
    assert (res.sweep.bad_waves, res.sweep.first_bad_wave) == (1, wave)
    r, t = recs[wave], wave // 4
    unit = f"xcc{r.xcc}.se{r.se}.sh0.cu{r.cu}.simd{wave % 4}"
    where = f"tile {t // 2},{t % 2} sub-tile {wave >> 1 & 1},{wave & 1}"
    assert f"mxgemm sweep: 1 of 24 waves wrong on 1 CU(s), first wave {wave} ({where}) on {unit}" \
        in cpu_agent._err()
    assert f"{unit} computed tile ({t // 2},{t % 2}) sub-tile ({wave >> 1 & 1},{wave & 1})" \
        in res.describe()


class FakeLib(GemmFakeLib):
    """The GEMM sweep's stand-in plus na_mxgemm_sweep. ``mx``: {(dev, format
    code): "sick" | "slow" | "noroom"}; default clean."""

    def __init__(self, ngpu=1, mx=None):
        super().__init__(ngpu=ngpu)
        self.mx_calls = []

        def na_mxgemm_sweep(dev, fmt, m, n, k, reps, seed, res, tflops):
            self.mx_calls.append((dev, fmt, m, n, k, reps, seed))
            kind = (mx or {}).get((dev, fmt), "ok")
            if kind == "noroom":
                self.error = b"na_mxgemm_sweep: the operands of 138412032 bytes do not fit: 1 bytes"
                return nodeagent.NA_ERR_ARG
            r = res._obj
            r.waves, r.units_seen, r.clock_mhz = 4096, 256, 2301.26 - fmt
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            tflops._obj.value = 1.5 if kind == "slow" else 2000.06 * (1 + fmt / 4)
            if kind != "sick":
                return 0
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 1, 1, 4 * 37 + 2, 1
            r.bad_list[0][:] = r.first_bad_unit[:] = (5, 2, 1, 9, 3)
            return nodeagent.NA_ERR_VERIFY

        self.na_mxgemm_sweep = na_mxgemm_sweep


def test_flag_reaches_check_through_the_cli(monkeypatch, capsys):
    monkeypatch.setattr(nodeagent, "MIN_MXGEMM_SWEEP_TFLOPS", {"fp8": 1500.0, "fp4": 3000.0})
    fakes = []
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fakes[-1])
    fakes.append(FakeLib())
    assert nodeagent.main([]) == 0 and fakes[-1].mx_calls == []
    capsys.readouterr()
    assert nodeagent.main(["--mxgemm-sweep"]) == 0
    assert fakes[-1].mx_calls == [(0, 0, 0, 0, 0, 0, SEED), (0, 4, 0, 0, 0, 0, SEED)]
    assert fakes[-1].gemm_calls == []
    g = json.loads(capsys.readouterr().out)["gpus"][0]
    assert [g[f"mxgemm_sweep_{f}"] for f in ("fp8_tflops", "fp4_tflops", "clock_mhz", "units_seen",
                                             "bad_waves", "skipped")] == [
        2000.1, 4000.1, 2301.3, 256, 0, ""]
    fakes.append(FakeLib(ngpu=2, mx={(1, 4): "sick"}))
    report = nodeagent.NodeAgent().check(mxgemm_sweep=True)
    assert report.problems == [
        "gpu1: MX GEMM sweep fp4: 1 of 4096 waves wrong on 1 CU(s): xcc5.se2.sh1.cu9 simd 3; first "
        "wave 150 on xcc5.se2.sh1.cu9.simd3 computed tile (1,5) sub-tile (1,0)"]
    assert report.gpus[1].mxgemm_sweep_bad_waves == 1
    assert nodeagent.node_condition_from_report(report)["status"] == "False"
    fakes.append(FakeLib(mx={(0, 0): "slow"}))
    assert nodeagent.NodeAgent().check(mxgemm_sweep=True).gpus[0].problems == [
        "MX GEMM sweep fp8 1.5 TFLOP/s below floor 1500.0"]
    fakes.append(FakeLib(mx={(0, 0): "noroom"}))
    g = nodeagent.NodeAgent().check(mxgemm_sweep=True).gpus[0]
    assert g.healthy and "do not fit" in g.mxgemm_sweep_skipped and g.mxgemm_sweep_fp8_tflops == 0.0


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _operands(agent, fmt, m, n, k):
    """a, b, sa, sb as uint8 tensors in the layout users' tensors have, filled."""
    per_byte = 2 if fmt == "fp4" else 1
    tensors = [torch.empty(shape, dtype=torch.uint8, device="cuda:0")
               for shape in [(m, k // per_byte), (n, k // per_byte), (m, k // 32), (n, k // 32)]]
    torch.cuda.synchronize()
    agent.mxgemm_sweep_fill(0, *(x.data_ptr() for x in tensors), m, n, k, SEED, fmt)
    return tensors


def _values(x, fmt):
    """The elements of an operand tensor; 99 for a code that is none of -3..3."""
    raw = x.cpu().numpy()
    if fmt == "fp4":  # the even k in the low nibble
        raw = np.stack([raw & 0xF, raw >> 4], axis=-1).reshape(raw.shape[0], -1)
    table = np.full(256, 99, dtype=np.int64)
    table[list(CODES[fmt])] = list(CODES[fmt].values())
    return table[raw]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape,reps", CASES)
def test_gpu_mxgemm(agent, shape, reps, fmt):
    m, n, k = shape[0], shape[1], shape[2] * BK[fmt]
    want_a, want_b, want_ea, want_eb, want_c, want_sums = ref(SEED, m, n, k, reps)
    a, b, sa, sb = _operands(agent, fmt, m, n, k)
    c = torch.full((m, n), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ptrs = [x.data_ptr() for x in (a, b, sa, sb)]
    recs, ms = agent.mxgemm_sweep_run(0, *ptrs, m, n, k, reps, SEED, fmt, c.data_ptr())
    print(f"{fmt} {m}x{n}x{k} reps {reps}: {ms:.3f} ms, SIMDs {[r.simd for r in recs]}")
    assert np.array_equal(_values(a, fmt), want_a) and np.array_equal(_values(b, fmt), want_b)
    assert np.array_equal(sa.cpu().numpy(), 127 + want_ea)
    assert np.array_equal(sb.cpu().numpy(), 127 + want_eb)
    assert np.array_equal(c.cpu().numpy().astype(np.int64), want_c)
    assert [r.checksum for r in recs] == want_sums
    assert [r.wave for r in recs] == list(range(len(want_sums)))
    rc, res = agent.mxgemm_sweep_verify(recs, m, n, k, reps, SEED, fmt)
    assert rc == nodeagent.NA_OK and res.sweep.bad_waves == 0, agent._err()
    for t in range(len(recs) // 4):
        four = recs[4 * t:4 * t + 4]
        assert len({(r.xcc, r.se, r.sh, r.cu) for r in four}) == 1
        assert sorted(r.simd for r in four) == [0, 1, 2, 3]
        assert all(r.cycles > 0 and r.realtime > 0 for r in four)
    again, _ms = agent.mxgemm_sweep_run(0, *ptrs, m, n, k, reps, SEED, fmt)
    assert [r.checksum for r in again] == want_sums


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("operand", ["sa", "sb"])
def test_gpu_one_changed_scale_byte_is_seen_by_the_waves_that_read_its_row(agent, fmt, operand):
    m, n, k = 768, 512, 2 * BK[fmt]
    block = BK[fmt] // 32 + 1  # in the second k-step
    a, b, sa, sb = _operands(agent, fmt, m, n, k)
    if operand == "sa":  # row 400: tile row 1, its lower half (wr 1), every tile column and wc
        sa[400, block] = 255 - sa[400, block]  # 127 <-> 128
        hit = [4 * (1 * 2 + tj) + 2 * 1 + wc for tj in range(2) for wc in range(2)]
    else:  # column 300: tile column 1, its left half (wc 0), every tile row and wr
        sb[300, block] = 255 - sb[300, block]
        hit = [4 * (ti * 2 + 1) + 2 * wr + 0 for ti in range(3) for wr in range(2)]
    torch.cuda.synchronize()
    recs, _ms = agent.mxgemm_sweep_run(0, *(x.data_ptr() for x in (a, b, sa, sb)), m, n, k, 1,
                                       SEED, fmt)
    rc, res = agent.mxgemm_sweep_verify(recs, m, n, k, 1, SEED, fmt)
    want = ref(SEED, m, n, k, 1)[5]
    assert [i for i, r in enumerate(recs) if r.checksum != want[i]] == hit
    assert rc == nodeagent.NA_ERR_VERIFY and res.sweep.bad_waves == len(hit)
    assert res.sweep.first_bad_wave == hit[0]
    assert ("tile 1,0 sub-tile 1,0" if operand == "sa" else "tile 0,1 sub-tile 0,0") in agent._err()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_default_sweep(agent, fmt):
    torch.cuda.synchronize()
    res = agent.mxgemm_sweep(0, fmt)
    _, _, _, cus = agent.device_info(0)
    print(f"mxgemm_sweep {fmt}: {res.tflops:.1f} TFLOP/s at {res.sweep.clock_mhz:.0f} MHz, "
          f"{res.sweep.units_seen} of {cus} CUs, {res.sweep.waves} waves")
    assert res.ok, res.describe()
    assert res.sweep.waves == 4 * 32 * 32 and res.sweep.units_seen == cus
    assert res.tflops >= nodeagent.MIN_MXGEMM_SWEEP_TFLOPS[fmt] > 0


@pytest.mark.gpu
def test_gpu_check_with_sweep(agent):
    torch.cuda.synchronize()
    report = agent.check(bw_bytes=1 << 28, mxgemm_sweep=True)
    g0 = report.gpus[0]
    assert g0.healthy, g0.problems
    assert g0.mxgemm_sweep_fp8_tflops >= nodeagent.MIN_MXGEMM_SWEEP_TFLOPS["fp8"]
    assert g0.mxgemm_sweep_fp4_tflops >= nodeagent.MIN_MXGEMM_SWEEP_TFLOPS["fp4"]
    assert g0.mxgemm_sweep_clock_mhz > 0 and g0.mxgemm_sweep_units_seen == g0.cus
    assert g0.mxgemm_sweep_bad_waves == 0 and g0.mxgemm_sweep_skipped == ""
