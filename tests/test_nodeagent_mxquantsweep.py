"""Chip-wide MX quantise sweep of the node agent (nodeagent/mxquantsweep.h): the
OCP MX quantiser, bf16 to MXFP8 / MXFP6 / MXFP4 and an E8M0 scale per 32
elements, on the gfx950 scaled conversion instructions.

The reference is the numpy copy of the specification below (``quantise``):
float64 arithmetic on the bf16 bit patterns, independent of the integer code
the library's own quantiser uses. The sign of a zero result follows the rule as
stated (the sign of the input); the hardware keeps it, so nothing deviates. The
GPU tests change one source element of their own tensor to see attribution: a
data mismatch; nothing on the GPU is provoked.
"""
import ctypes
import functools
import json

import numpy as np
import pytest

# torch first, before any test loads the agent library: see the note at the
# top of test_nodeagent_memtest.py (one HIP runtime per process -- torch's).
try:
    import torch
except ImportError:  # CPU-only environment: the GPU tests cannot run there
    torch = None

from gpu_provisioner_amd import nodeagent
from tests.test_nodeagent_gemmsweep import _ensure_lib
from tests.test_nodeagent_mfmasweep import _mix64
from tests.test_nodeagent_mxgemmsweep import FakeLib as MxGemmFakeLib
from tests.test_nodeagent_mxgemmsweep import ref as gemm_ref

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
U64 = np.uint64
SEED = getattr(nodeagent, "DEFAULT_MXQUANT_SWEEP_SEED", 0)
FORMATS = ["fp8", "fp6", "fp4"]
# bits, mantissa bits, exponent bias, emax, largest finite magnitude
SPEC = {"fp8": (8, 3, 7, 8, 448.0), "fp6": (6, 3, 1, 2, 7.5), "fp4": (4, 1, 1, 2, 6.0)}
SHAPES = [(1, 32), (3, 96), (5, 160), (257, 32), (64, 4128)]  # B = 1, 9, 25, 257, 8256


def quantise(src, fmt):
    """(dst, scales) of the specification for src, uint16[B][32] of bf16 patterns."""
    bits, man, bias, emax, top = SPEC[fmt]
    mag = (src & 0x7FFF).astype(np.int64)
    value = np.ldexp(1 + (mag & 127) / 128.0, (mag >> 7) - 127) * (mag >> 7 != 0)
    amax = value.max(axis=1)
    e = np.where(amax > 0, np.frexp(amax)[1] - 1 - emax, 0)  # floor(log2 amax) - emax
    scales = np.where(amax > 0, 127 + e, 0).astype(np.uint8)
    y = np.ldexp(value, -e[:, None])
    # nearest even on the format's grid: steps of 2^(exponent - man), the
    # exponent no lower than the smallest normal's; then saturate
    step = np.maximum(np.frexp(y)[1] - 1, 1 - bias) - man
    q = np.minimum(np.ldexp(np.rint(np.ldexp(y, -step)), step), top)
    qe = np.maximum(np.frexp(q)[1] - 1, 1 - bias)
    # subnormals count steps from 0, normals from (exponent field << man) with the implicit one
    code = (np.ldexp(q, man - qe) + (qe + bias - 1) * (1 << man) * (q >= 2.0 ** (1 - bias)))
    code = code.astype(np.int64) | (src >> 15).astype(np.int64) << (bits - 1)
    stream = (code[:, :, None] >> np.arange(bits) & 1).astype(np.uint8).reshape(len(src), -1)
    return np.packbits(stream, axis=1, bitorder="little"), scales


def source(seed, blocks):
    """The sweep's hashed source, uint16[blocks][32]."""
    with np.errstate(over="ignore"):
        base, i = U64(seed * G & M64), np.arange(blocks * 32, dtype=U64)
        x, h = i >> U64(5), _mix64(base + i)
        binade = ((_mix64(base + U64(blocks * 32) + x) >> U64(40)) % U64(41)).astype(np.int64) - 20
    ex = 127 + binade - ((h >> U64(32)) % U64(11)).astype(np.int64)
    bits = ((h >> U64(11) & U64(1)).astype(np.int64) << 15 | ex << 7
            | (h >> U64(4) & U64(127)).astype(np.int64))
    zero = (x % U64(64) == 63) | (h % U64(16) == 0)
    return np.where(zero, 0, bits).astype(np.uint16).reshape(blocks, 32)


def checksums(dst, scales, seed, workgroups, passes):
    """The checksum formula on a quantiser's output: 4 * workgroups sums."""
    words, x = dst.view("<u4").astype(U64), np.arange(len(dst), dtype=U64)
    out = np.zeros(4 * workgroups, dtype=U64)
    with np.errstate(over="ignore"):
        h = scales.astype(U64)
        for i in range(words.shape[1]):
            h = (U64(33) * h + words[:, i]) & U64(0xFFFFFFFF)
        weight = _mix64(U64(seed * G & M64) + x) | U64(1)
        np.add.at(out, (x // U64(256) % U64(workgroups) * U64(4) + x % U64(256) // U64(64))
                  .astype(np.int64), U64(passes) * weight * h)
    return [int(v) for v in out]


@functools.lru_cache(maxsize=None)
def exhaustive():
    """Every bf16 pattern p inside the contract (normal or zero) at slot p % 32
    of a block of its own, next to a companion 2^(E_p + j) for j in 0, 1, 4, 9,
    kept within 2^-100 .. 2^127, zeros elsewhere."""
    p = np.arange(1 << 16)
    p = p[((p >> 7 & 255) % 255 != 0) | (p & 0x7FFF == 0)]
    rows, blocks = np.arange(len(p)), []
    for j in (0, 1, 4, 9):
        b = np.zeros((len(p), 32), dtype=np.uint16)
        b[rows, p % 32] = p
        b[rows, (p + 1) % 32] = np.clip((p >> 7 & 255) + j, 27, 254) << 7
        blocks.append(b)
    return np.concatenate(blocks)


@functools.lru_cache(maxsize=None)
def exhaustive_want(fmt):
    return quantise(exhaustive(), fmt)


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


def _reference(cpu_agent, src, fmt):
    dst, scales = cpu_agent.mxquant_reference(src.tobytes(), len(src), 32, fmt)
    return np.frombuffer(dst, np.uint8).reshape(len(src), -1), np.frombuffer(scales, np.uint8)


@pytest.mark.parametrize("fmt", FORMATS)
def test_reference_matches_numpy_on_every_pattern(cpu_agent, fmt):
    assert list(nodeagent.MXQUANT_FORMATS) == FORMATS
    dst, scales = _reference(cpu_agent, exhaustive(), fmt)
    want_dst, want_scales = exhaustive_want(fmt)
    assert np.array_equal(scales, want_scales) and np.array_equal(dst, want_dst)
    if fmt == "fp8":  # saturation and -0 are in there, a NaN code is not
        assert 0x7E in dst and 0xFE in dst and 0x80 in dst and 0x7F not in dst and 0xFF not in dst


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("blocks", [1, 255, 257, 1030])
@pytest.mark.parametrize("workgroups,passes", [(1, 1), (3, 2)])
def test_expected_is_the_checksum_of_the_reference_on_the_hashed_source(
        cpu_agent, fmt, blocks, workgroups, passes):
    src = source(SEED, blocks)
    dst, scales = _reference(cpu_agent, src, fmt)
    assert np.array_equal(dst, quantise(src, fmt)[0])
    assert len(set(scales)) > min(blocks, 20) // 2 and (scales[63::64] == 0).all()  # binades vary
    assert cpu_agent.mxquant_expected(blocks, 32, workgroups, passes, SEED, fmt) == checksums(
        dst, scales, SEED, workgroups, passes)


@pytest.mark.parametrize("fmt,rows,k,workgroups,passes", [
    (1, 4, 64, 1, 1), (3, 4, 64, 1, 1), (5, 4, 64, 1, 1), (-1, 4, 64, 1, 1),  # no such format
    (0, 4, 48, 1, 1), (0, 4, 0, 1, 1), (0, 0, 64, 1, 1), (0, -1, 64, 1, 1),
    (0, 1 << 20, 1024, 1, 1),  # 2^25 blocks
    (0, 4, 64, 0, 1), (0, 4, 64, 1, 0), (0, 4, 64, 1, (1 << 20) + 1)])
def test_argument_errors_before_any_hip_call(cpu_agent, fmt, rows, k, workgroups, passes):
    lib, bad, ptr = cpu_agent.lib, nodeagent.NA_ERR_ARG, 1 << 40  # never followed
    recs, out = (nodeagent.MfmaRecord * 8)(), (ctypes.c_uint64 * 8)()
    res = nodeagent._MfmaSweepResultC()
    assert lib.na_mxquant_run(0, fmt, ptr, ptr, ptr, rows, k, workgroups, passes, SEED, recs, 8,
                              None) == bad
    assert "na_mxquant_run" in cpu_agent._err()
    assert lib.na_mxquant_expected(fmt, SEED, rows, k, workgroups, passes, out, 8) == bad
    assert lib.na_mxquant_verify(recs, 4 * workgroups, fmt, rows, k, workgroups, passes, SEED,
                                 ctypes.byref(res)) == bad
    if workgroups == 1 and passes == 1:
        assert lib.na_mxquant_reference(fmt, ptr, rows, k, ptr, ptr) == bad
        if fmt == 0:
            assert lib.na_mxquant_fill(0, ptr, rows, k, SEED) == bad
    else:
        assert lib.na_mxquant_sweep(0, fmt, -workgroups, -passes or -1, SEED, ctypes.byref(res),
                                    None) == bad


def test_pointer_and_buffer_errors_before_any_hip_call(cpu_agent):
    lib, bad, ptr = cpu_agent.lib, nodeagent.NA_ERR_ARG, 1 << 40
    recs = (nodeagent.MfmaRecord * 8)()
    for src, dst, scales, n in [(None, ptr, ptr, 8), (ptr + 8, ptr, ptr, 8), (ptr, ptr + 4, ptr, 8),
                                (ptr, ptr, ptr + 2, 8), (ptr, ptr, None, 8), (ptr, ptr, ptr, 7)]:
        assert lib.na_mxquant_run(0, 0, src, dst, scales, 4, 64, 2, 1, SEED, recs, n, None) == bad
    assert lib.na_mxquant_run(0, 0, ptr, ptr, ptr, 4, 64, 2, 1, SEED, None, 8, None) == bad
    assert lib.na_mxquant_fill(0, ptr + 2, 4, 64, SEED) == bad
    assert lib.na_mxquant_expected(0, SEED, 4, 64, 2, 1, (ctypes.c_uint64 * 7)(), 7) == bad
    assert lib.na_mxquant_sweep(0, 0, 0, 0, SEED, None, None) == bad
    with pytest.raises(nodeagent.NodeAgentError, match="'bf8' is not one of fp8, fp6, fp4"):
        cpu_agent.mxquant_sweep(0, "bf8")


class FakeLib(MxGemmFakeLib):
    """The MX GEMM sweep's stand-in plus na_mxquant_sweep. ``quant``: {(dev,
    format code): "sick" | "slow"}; default clean."""

    def __init__(self, ngpu=1, quant=None):
        super().__init__(ngpu=ngpu)
        self.quant_calls = []

        def na_mxquant_sweep(dev, fmt, workgroups, passes, seed, res, gelems):
            self.quant_calls.append((dev, fmt, workgroups, passes, seed))
            kind = (quant or {}).get((dev, fmt), "ok")
            r = res._obj
            r.waves, r.units_seen, r.clock_mhz = 4096, 256, 2301.26 - fmt
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            gelems._obj.value = 1.5 if kind == "slow" else 3000.06 + fmt
            if kind != "sick":
                return 0
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 1, 1, 4 * 37 + 2, 1
            r.bad_list[0][:] = r.first_bad_unit[:] = (5, 2, 1, 9, 3)
            return nodeagent.NA_ERR_VERIFY

        self.na_mxquant_sweep = na_mxquant_sweep


def test_flag_reaches_check_through_the_cli(monkeypatch, capsys):
    monkeypatch.setattr(nodeagent, "MIN_MXQUANT_SWEEP_GELEMS", dict.fromkeys(FORMATS, 2500.0))
    fakes = []
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fakes[-1])
    fakes.append(FakeLib())
    assert nodeagent.main([]) == 0 and fakes[-1].quant_calls == []
    capsys.readouterr()
    assert nodeagent.main(["--mxquant-sweep"]) == 0
    assert fakes[-1].quant_calls == [(0, code, 0, 0, SEED) for code in (0, 2, 4)]
    assert fakes[-1].mx_calls == []
    g = json.loads(capsys.readouterr().out)["gpus"][0]
    assert [g[f"mxquant_sweep_{f}"] for f in ("fp8_gelems", "fp6_gelems", "fp4_gelems", "clock_mhz",
                                              "units_seen", "bad_waves")] == [
        3000.1, 3002.1, 3004.1, 2301.3, 256, 0]
    fakes.append(FakeLib(ngpu=2, quant={(1, 2): "sick"}))
    report = nodeagent.NodeAgent().check(mxquant_sweep=True)
    assert report.problems == [
        "gpu1: MX quantise sweep fp6: 1 of 4096 waves wrong on 1 CU(s): xcc5.se2.sh1.cu9 simd 3; "
        "first wave 150 (workgroup 37 wave 2) on xcc5.se2.sh1.cu9.simd3"]
    assert report.gpus[1].mxquant_sweep_bad_waves == 1
    assert nodeagent.node_condition_from_report(report)["status"] == "False"
    fakes.append(FakeLib(quant={(0, 4): "slow"}))
    assert nodeagent.NodeAgent().check(mxquant_sweep=True).gpus[0].problems == [
        "MX quantise sweep fp4 1.5 Gelem/s (conversion rate) below floor 2500.0"]


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


GUARD = 0xA5


def _run(agent, src, fmt, workgroups, passes=1, seed=SEED):
    """src (uint16[B][32]) through na_mxquant_run: (dst, scales, records, source
    tensor), the outputs with 64 guard bytes behind them."""
    blocks, width = len(src), 4 * SPEC[fmt][0]
    d_src = src if torch.is_tensor(src) else torch.from_numpy(src.view(np.int16)).to("cuda:0")
    dst = torch.full((blocks * width + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    scales = torch.full((blocks + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    recs, _ms = agent.mxquant_run(0, d_src.data_ptr(), dst.data_ptr(), scales.data_ptr(), blocks,
                                  32, workgroups, passes, seed, fmt)
    return dst.cpu().numpy(), scales.cpu().numpy(), recs, d_src


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_every_bf16_pattern_at_four_distances_from_amax(agent, fmt):
    src, (want_dst, want_scales) = exhaustive(), exhaustive_want(fmt)
    dst, scales, _recs, _src = _run(agent, src, fmt, 64)
    dst = dst[:-64].reshape(len(src), -1)
    wrong = np.flatnonzero((dst != want_dst).any(axis=1) | (scales[:-64] != want_scales))
    for x in wrong[:20]:
        print(f"{fmt} block {x}: pattern {src[x].max():#06x} got {bytes(dst[x]).hex()} scale "
              f"{scales[x]}, want {bytes(want_dst[x]).hex()} scale {want_scales[x]}")
    assert len(wrong) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("rows,k", SHAPES)
@pytest.mark.parametrize("workgroups,passes", [(1, 1), (3, 2)])
def test_gpu_shapes(agent, fmt, rows, k, workgroups, passes):
    blocks, width = rows * k // 32, 4 * SPEC[fmt][0]
    d_src = torch.empty((blocks, 32), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    agent.mxquant_fill(0, d_src.data_ptr(), rows, k, SEED)
    src = d_src.cpu().numpy().view(np.uint16)
    assert np.array_equal(src, source(SEED, blocks))
    dst, scales, recs, _src = _run(agent, d_src, fmt, workgroups, passes)
    want_dst, want_scales = quantise(src, fmt)
    assert np.array_equal(dst[:-64].reshape(blocks, width), want_dst)
    assert np.array_equal(scales[:-64], want_scales)
    assert (dst[-64:] == GUARD).all() and (scales[-64:] == GUARD).all()
    assert [r.checksum for r in recs] == checksums(want_dst, want_scales, SEED, workgroups, passes)
    rc, res = agent.mxquant_verify(recs, rows, k, workgroups, passes, SEED, fmt)
    assert rc == nodeagent.NA_OK and res.ok and res.sweep.waves == 4 * workgroups, agent._err()
    assert sorted(r.simd for r in recs[:4]) == [0, 1, 2, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_a_changed_scale_is_pinned_on_the_wave_that_owns_the_block(agent, fmt):
    rows, k, workgroups, x = 64, 4128, 3, 5000  # tile 19: workgroup 19 % 3, wave (5000 % 256) / 64
    src = source(SEED, rows * k // 32)
    _dst, scales, recs, _src = _run(agent, src, fmt, workgroups)
    assert agent.mxquant_verify(recs, rows, k, workgroups, 1, SEED, fmt)[0] == nodeagent.NA_OK
    src[x, 0] = 0x4E80  # 2^30: far above the block's binade
    _dst, changed, recs, _src = _run(agent, src, fmt, workgroups)
    assert changed[x] != scales[x] and np.array_equal(np.delete(changed, x), np.delete(scales, x))
    rc, res = agent.mxquant_verify(recs, rows, k, workgroups, 1, SEED, fmt)
    assert rc == nodeagent.NA_ERR_VERIFY and res.sweep.bad_waves == 1
    assert res.sweep.first_bad_wave == 4 * (19 % 3) + 2
    assert f"first wave 6 (workgroup 1 wave 2) on {nodeagent.mfma_unit_name(res.sweep.bad_simds[0])}" \
        in agent._err()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_gpu_quantised_operands_pass_the_mx_gemm_sweep(agent, fmt):
    m, n, k, seed = 256, 256, 512, nodeagent.DEFAULT_MXGEMM_SWEEP_SEED
    a, b, ea, eb, _c, _sums = gemm_ref(seed, m, n, k, 1)
    ptrs, keep = [], []
    for values, exps in [(a, ea), (b, eb)]:
        scaled = (values << np.repeat(exps, 32, axis=1)).astype(np.float32)  # exact in bf16
        src = (scaled.view(np.uint32) >> 16).astype(np.uint16).reshape(-1, 32)
        width = 4 * SPEC[fmt][0]
        d_src = torch.from_numpy(src.view(np.int16)).to("cuda:0")
        dst = torch.empty((len(src) * width,), dtype=torch.uint8, device="cuda:0")
        scales = torch.empty((len(src),), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        agent.mxquant_run(0, d_src.data_ptr(), dst.data_ptr(), scales.data_ptr(), m, k, 3, 1, seed, fmt)
        want = 127 + exps.reshape(-1) + (1 - SPEC[fmt][3])  # OCP: 3 * 2^ea has exponent ea + 1
        assert np.array_equal(scales.cpu().numpy()[np.abs(values).reshape(-1, 32).max(axis=1) >= 2],
                              want[np.abs(values).reshape(-1, 32).max(axis=1) >= 2])
        ptrs += [dst.data_ptr(), scales.data_ptr()]
        keep += [d_src, dst, scales]
    recs, _ms = agent.mxgemm_sweep_run(0, ptrs[0], ptrs[2], ptrs[1], ptrs[3], m, n, k, 1, seed, fmt)
    rc, res = agent.mxgemm_sweep_verify(recs, m, n, k, 1, seed, fmt)
    assert rc == nodeagent.NA_OK and res.ok, agent._err()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_gpu_default_sweep(agent, fmt):
    torch.cuda.synchronize()
    res = agent.mxquant_sweep(0, fmt)
    _, _, _, cus = agent.device_info(0)
    print(f"mxquant_sweep {fmt}: {res.gelems:.1f} Gelem/s (conversion rate, not a memory figure) "
          f"at {res.sweep.clock_mhz:.0f} MHz, {res.sweep.units_seen} of {cus} CUs")
    assert res.ok, res.describe()
    assert res.sweep.waves == 16 * cus and res.sweep.units_seen == cus
    # the SIMDs, from the records of one pass over a source of the sweep's shape
    d_src = torch.empty((16 * cus * 256, 32), dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    agent.mxquant_fill(0, d_src.data_ptr(), 16 * cus, 8192, SEED)
    recs = _run(agent, d_src, fmt, 4 * cus)[2]
    assert len({(r.xcc, r.se, r.sh, r.cu, r.simd) for r in recs}) == 4 * cus
    assert res.gelems >= nodeagent.MIN_MXQUANT_SWEEP_GELEMS[fmt] > 0
