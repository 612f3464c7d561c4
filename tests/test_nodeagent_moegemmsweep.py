"""Chip-wide MoE grouped GEMM sweep of the node agent (nodeagent/moegemmsweep.h):
C[s] = reps * X[row_ids[s]] * W[e]^T for the slots s of expert e, rows gathered
through an index array, ragged counts per expert, tiles found on the device.

The reference is the numpy copy of the specification below: operands from the
hash, a plain float64 product per slot, every wave's checksum as the direct sum
of p_s * q_j * C[s][j] over its valid rows. It shares nothing with the host
code's U/V dot products. The GPU tests change an element of their own tensors
to see detection: a data mismatch; nothing on the GPU is provoked.
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
from tests.test_nodeagent_gemmsweep import BK, E4M3, G, M64, U64, _ensure_lib, _values
from tests.test_nodeagent_mfmasweep import FakeLib as MfmaFakeLib
from tests.test_nodeagent_mfmasweep import _mix64

SEED = getattr(nodeagent, "DEFAULT_MOE_GEMM_SWEEP_SEED", 0)
TOKENS = 300  # fewer than most slot counts: row ids repeat
# one full tile; a single slot; one short of a tile; a second tile of one row;
# empty experts at both ends; a mixed ragged set; no tile at all; more tiles
# than 8 XCDs and the wrap of the block map
COUNTS = [(128,), (1,), (127,), (129,), (0, 5, 0), (130, 0, 1, 256, 77), (0, 0),
          tuple(64 + 37 * i % 137 for i in range(20))]


def slots_of(counts):
    return sum(counts) + 3  # three dropped tokens behind the last expert


def bound_of(counts, n):
    return (slots_of(counts) // 128 + len(counts)) * (n // 256)


@functools.lru_cache(maxsize=None)
def ref(seed, counts, n, k, reps):
    """(X, W, row_ids, C with -1 in the rows nobody owns, checksums)."""
    slots, experts = slots_of(counts), len(counts)
    with np.errstate(over="ignore"):
        def hashed(first, count):
            return _mix64(U64((seed * G + first) & M64) + np.arange(count, dtype=U64))

        x = ((hashed(0, TOKENS * k) >> U64(40)) % U64(7)).astype(np.int64).reshape(TOKENS, k) - 3
        w = ((hashed(TOKENS * k, experts * n * k) >> U64(40)) % U64(5)).astype(np.int64) - 2
        w = w.reshape(experts, n, k)
        p = hashed(TOKENS * k + experts * n * k, slots) | U64(1)
        q = hashed(TOKENS * k + experts * n * k + slots, n) | U64(1)
        ids = (_mix64(U64((seed * G - 1) & M64) - np.arange(slots, dtype=U64))
               % U64(TOKENS)).astype(np.int64)
        c = np.full((slots, n), -1.0)
        sums, tile, s0 = [0] * (4 * bound_of(counts, n)), 0, 0
        for e, cnt in enumerate(counts):
            # small integers: the float64 product is exact
            c[s0:s0 + cnt] = reps * (x[ids[s0:s0 + cnt]].astype(np.float64) @ w[e].T.astype(np.float64))
            for r0 in range(s0, s0 + cnt, 128):
                for tj in range(n // 256):
                    for wave in range(4):
                        rows = slice(r0 + 64 * (wave >> 1), min(r0 + 64 * (wave >> 1) + 64, s0 + cnt))
                        cols = slice(256 * tj + 128 * (wave & 1), 256 * tj + 128 * (wave & 1) + 128)
                        part = p[rows, None] * q[None, cols] * c[rows, cols].astype(np.int64).astype(U64)
                        sums[4 * tile + wave] = int(part.sum(dtype=U64))
                    tile += 1
            s0 += cnt
    return x, w, ids, c, sums


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("reps", [1, 3])
@pytest.mark.parametrize("n", [256, 512])
@pytest.mark.parametrize("ksteps", [1, 2, 3])
@pytest.mark.parametrize("counts", COUNTS)
def test_expected_matches_direct_sum(cpu_agent, counts, ksteps, n, reps, dtype):
    k, slots = ksteps * BK[dtype], slots_of(counts)
    assert cpu_agent.moe_gemm_tiles(slots, len(counts), n) == bound_of(counts, n)
    assert cpu_agent.moe_gemm_expected(TOKENS, slots, n, k, counts, reps, SEED) \
        == ref(SEED, counts, n, k, reps)[4]
    if counts == COUNTS[5] and ksteps == 1:  # and a seed past 2^40, whose high half matters
        big = (1 << 40) + 9
        got = cpu_agent.moe_gemm_expected(TOKENS, slots, n, k, counts, reps, big)
        assert got == ref(big, counts, n, k, reps)[4]
        assert got != cpu_agent.moe_gemm_expected(TOKENS, slots, n, k, counts, reps, big & 0xFFFFFFFF)


@pytest.mark.parametrize("tokens,slots,counts,n,k,reps,n_delta", [
    (0, 8, (5,), 256, 64, 1, 0),          # no tokens
    (300, 0, (0,), 256, 64, 1, 0),        # no slots
    (300, 8, (5,) * 257, 256, 64, 1, 0),  # more than 256 experts
    (300, 8, (5,), 384, 64, 1, 0),        # N no multiple of 256
    (300, 8, (5,), 256, 96, 1, 0),        # K no multiple of 64
    (300, 8, (5,), 256, 8192, 342, 0),    # 6 * reps * K = 2^24 and more
    (300, 8, (5, 4), 256, 64, 1, 0),      # counts beyond the slots
    (300, 8, (5, -1), 256, 64, 1, 0),     # a negative count
    (300, 8, (5,), 256, 64, 1, 4),        # a record buffer of the wrong size
])
def test_argument_errors_before_any_hip_call(cpu_agent, tokens, slots, counts, n, k, reps, n_delta):
    lib, experts, bad = cpu_agent.lib, len(counts), nodeagent.NA_ERR_ARG
    size = 4 * (max(slots, 1) // 128 + experts) * max(n // 256, 1) + n_delta
    out, recs, res = (ctypes.c_uint64 * size)(), (nodeagent.MfmaRecord * size)(), nodeagent._MfmaSweepResultC()
    cnts, ptr = (ctypes.c_int * experts)(*counts), 1 << 40  # the pointer is never followed
    assert lib.na_moe_gemm_expected(SEED, tokens, slots, experts, n, k, cnts, reps, out, size) == bad
    assert "na_moe_gemm_expected" in cpu_agent._err()
    assert lib.na_moe_gemm_verify(recs, size, tokens, slots, experts, n, k, cnts, reps, SEED,
                                  ctypes.byref(res)) == bad
    assert "na_moe_gemm_verify" in cpu_agent._err()
    # a device that does not exist: the arguments are refused before it is looked at
    if min(counts) >= 0 and sum(counts) <= slots:  # the run sees the counts on the device only
        assert lib.na_moe_gemm_run(99, 0, ptr, ptr, ptr, ptr, None, tokens, slots, experts, n, k,
                                   reps, SEED, recs, size, None) == bad
        assert "na_moe_gemm_run" in cpu_agent._err()
    if reps == 1 and not n_delta:  # the fill takes neither repetitions nor records
        assert lib.na_moe_gemm_fill(99, 0, ptr, ptr, ptr, ptr, tokens, slots, experts, n, k, cnts,
                                    SEED) == bad
        assert "na_moe_gemm_fill" in cpu_agent._err()
    if n_delta:  # everything else is in order: the pointers and the dtype are looked at
        for args in [(0, ptr + 8, ptr, ptr, ptr), (0, ptr, ptr, ptr + 2, ptr), (0, ptr, None, ptr, ptr),
                     (2, ptr, ptr, ptr, ptr), (1, ptr, ptr, ptr, ptr)]:  # fp8 needs K of 128
            assert lib.na_moe_gemm_run(99, *args, None, tokens, slots, experts, n, k, reps, SEED,
                                       recs, size - n_delta, None) == bad, args
        assert lib.na_moe_gemm_sweep(99, 0, 0, 0, 257, 0, 0, 0, SEED, ctypes.byref(res), None) == bad
        assert lib.na_moe_gemm_sweep(99, 0, 0, 0, 0, 0, 0, 0, SEED, None, None) == bad
        assert lib.na_moe_gemm_tiles(slots, experts, n, None) == bad


def test_verify_names_the_wave_and_wants_the_surplus_idle(cpu_agent):
    counts, n, k = COUNTS[5], 512, 128
    slots, want = slots_of(counts), ref(SEED, counts, n, k, 2)[4]
    recs = (nodeagent.MfmaRecord * len(want))()
    for i, r in enumerate(recs):
        r.checksum, r.wave, r.cycles, r.realtime = want[i], i, 21000, 1000
        r.xcc, r.se, r.sh, r.cu, r.simd = i // 4 % 8, i // 32 % 4, 0, i // 4 % 16, i % 4
    rc, res = cpu_agent.moe_gemm_verify(recs, TOKENS, slots, n, k, counts, 2, SEED)
    assert rc == nodeagent.NA_OK and res.ok and res.sweep.waves == 4 * bound_of(counts, n)
    # row tiles 2 + 0 + 1 + 2 + 1, two column tiles: record 4 * (3 * 2 + 1) + 2 is
    # expert 3's first row tile, column tile 1, sub-tile (1, 0); 4 * 12 is the first idle one
    for wave, where in [(30, "expert 3 row tile 0 column tile 1 sub-tile 1,0"),
                        (48, "a surplus workgroup that must report idle")]:
        recs[wave].checksum ^= 1 << 17
        rc, res = cpu_agent.moe_gemm_verify(recs, TOKENS, slots, n, k, counts, 2, SEED)
        recs[wave].checksum ^= 1 << 17
        assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
        assert (res.sweep.bad_waves, res.sweep.first_bad_wave) == (1, wave)
        unit = f"xcc{recs[wave].xcc}.se{recs[wave].se}.sh0.cu{recs[wave].cu}.simd{wave % 4}"
        assert f"first record {wave} ({where}) on {unit}" in cpu_agent._err()
        assert where.split(" sub-tile")[0] in res.describe() and unit in res.describe()


class FakeLib(MfmaFakeLib):
    """The matrix-core sweep's stand-in plus na_moe_gemm_sweep. ``moe``: {dev:
    "sick" | "slow" | "noroom"}; default clean."""

    def __init__(self, ngpu=1, moe=None):
        super().__init__(ngpu=ngpu)
        self.moe_calls = []

        def na_moe_gemm_sweep(dev, dtype, tokens, slots, experts, n, k, reps, seed, res, tflops):
            self.moe_calls.append((dev, dtype, tokens, slots, experts, n, k, reps, seed))
            kind = (moe or {}).get(dev, "ok")
            if kind == "noroom":
                self.error = b"na_moe_gemm_sweep: the operands of 268435456 bytes do not fit: 1 bytes"
                return nodeagent.NA_ERR_ARG
            r = res._obj
            r.waves, r.units_seen, r.clock_mhz = 9216, 256, 1801.26
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            tflops._obj.value = 1.5 if kind == "slow" else 601.26
            if kind != "sick":
                return 0
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 1, 1, 4 * 37 + 2, 1
            r.bad_list[0][:] = r.first_bad_unit[:] = (5, 2, 1, 9, 3)
            self.error = b"moe gemm sweep: first record 150 (expert 2 row tile 1 ...)"
            return nodeagent.NA_ERR_VERIFY

        self.na_moe_gemm_sweep = na_moe_gemm_sweep


def test_flag_reaches_check_through_the_cli(monkeypatch, capsys):
    monkeypatch.setattr(nodeagent, "MIN_MOE_GEMM_SWEEP_TFLOPS", 400.0)
    fakes = []
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fakes[-1])
    fakes.append(FakeLib())
    assert nodeagent.main([]) == 0 and fakes[-1].moe_calls == []
    capsys.readouterr()
    assert nodeagent.main(["--moe-gemm-sweep"]) == 0
    assert fakes[-1].moe_calls == [(0, 0, 0, 0, 0, 0, 0, 0, SEED)] and fakes[-1].sweep_calls == []
    g = json.loads(capsys.readouterr().out)["gpus"][0]
    assert [g[f"moe_gemm_sweep_{f}"] for f in ("tflops", "clock_mhz", "units_seen", "bad_waves",
                                               "skipped")] == [601.3, 1801.3, 256, 0, ""]
    fakes.append(FakeLib(ngpu=2, moe={1: "sick"}))
    report = nodeagent.NodeAgent().check(moe_gemm_sweep=True)
    assert report.problems == [
        "gpu1: MoE GEMM sweep: 1 of 9216 waves wrong on 1 CU(s): xcc5.se2.sh1.cu9 simd 3; first "
        "record 150 (tile 37 sub-tile 1,0) on xcc5.se2.sh1.cu9.simd3; moe gemm sweep: first record "
        "150 (expert 2 row tile 1 ...)"]
    assert nodeagent.node_condition_from_report(report)["status"] == "False"
    fakes.append(FakeLib(moe={0: "slow"}))
    assert nodeagent.NodeAgent().check(moe_gemm_sweep=True).gpus[0].problems == [
        "MoE GEMM sweep 1.5 TFLOP/s below floor 400.0"]
    fakes.append(FakeLib(moe={0: "noroom"}))
    g = nodeagent.NodeAgent().check(moe_gemm_sweep=True).gpus[0]
    assert g.healthy and "do not fit" in g.moe_gemm_sweep_skipped and g.moe_gemm_sweep_tflops == 0.0


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _filled(agent, dtype, counts, n, k):
    """(X, W, row_ids, offsets) of the sweep on the GPU."""
    kind = torch.bfloat16 if dtype == "bf16" else torch.uint8
    x = torch.empty((TOKENS, k), dtype=kind, device="cuda:0")
    w = torch.empty((len(counts), n, k), dtype=kind, device="cuda:0")
    ids = torch.empty((slots_of(counts),), dtype=torch.int32, device="cuda:0")
    offsets = torch.empty((len(counts) + 1,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    agent.moe_gemm_fill(0, x.data_ptr(), w.data_ptr(), ids.data_ptr(), offsets.data_ptr(), TOKENS,
                        len(ids), n, k, counts, SEED, dtype)
    return x, w, ids, offsets


def _run(agent, dtype, x, w, ids, offsets, reps=1):
    """(records, C prefilled with -1) of one launch."""
    c = torch.full((len(ids), w.shape[1]), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    recs, _ms = agent.moe_gemm_run(0, x.data_ptr(), w.data_ptr(), ids.data_ptr(), offsets.data_ptr(),
                                   x.shape[0], len(ids), w.shape[0], w.shape[1], x.shape[1], reps,
                                   SEED, dtype, c.data_ptr())
    return recs, c.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("counts", COUNTS)
def test_gpu_every_record_and_c_are_exact(agent, counts, dtype):
    n, k, reps = 512, 3 * BK[dtype], 2
    want_x, want_w, want_ids, want_c, want_sums = ref(SEED, counts, n, k, reps)
    x, w, ids, offsets = _filled(agent, dtype, counts, n, k)
    assert np.array_equal(_values(x, dtype), want_x) and np.array_equal(_values(w, dtype), want_w)
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    assert offsets.tolist() == [sum(counts[:e]) for e in range(len(counts) + 1)]
    recs, c = _run(agent, dtype, x, w, ids, offsets, reps)
    # the dropped slots behind the last expert keep their -1; a tail tile's rows past
    # its expert's count hold the NEXT expert's product
    assert np.array_equal(c, want_c)
    assert [r.checksum for r in recs] == want_sums
    assert [r.wave for r in recs] == list(range(4 * bound_of(counts, n)))  # idle ones too
    rc, res = agent.moe_gemm_verify(recs, TOKENS, len(ids), n, k, counts, reps, SEED, dtype)
    assert rc == nodeagent.NA_OK and res.sweep.bad_waves == 0, agent._err()
    for t in range(len(recs) // 4):
        four = recs[4 * t:4 * t + 4]
        assert len({(r.xcc, r.se, r.sh, r.cu) for r in four}) == 1
        assert sorted(r.simd for r in four) == [0, 1, 2, 3]
        assert all(r.cycles > 0 and r.realtime > 0 for r in four)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_gpu_a_changed_weight_or_row_id_fails_exactly_the_waves_that_read_it(agent, dtype):
    counts, n, k = COUNTS[5], 512, 2 * BK[dtype]
    x, w, ids, offsets = _filled(agent, dtype, counts, n, k)
    want = ref(SEED, counts, n, k, 1)[4]

    def bad(recs):
        return [i for i, r in enumerate(recs) if r.checksum != want[i]]

    # W[3][400]: expert 3 is row tiles 3 and 4, row 400 column tile 1, wc 1; both wr
    e, j, col = 3, 400, BK[dtype] + 17
    was = int(_values(w[e, j:j + 1, col:col + 1], dtype)[0, 0])
    now = 1 if was != 1 else 2  # another small integer, exact in both formats
    w[e, j, col] = now if dtype == "bf16" else next(c for c, v in E4M3.items() if v == now)
    recs, _c = _run(agent, dtype, x, w, ids, offsets)
    assert bad(recs) == [4 * (rt * 2 + 1) + 2 * wr + 1 for rt in (3, 4) for wr in (0, 1)]
    rc, res = agent.moe_gemm_verify(recs, TOKENS, len(ids), n, k, counts, 1, SEED, dtype)
    assert rc == nodeagent.NA_ERR_VERIFY and res.sweep.bad_waves == 4
    assert "expert 3 row tile 0 column tile 1 sub-tile 0,1" in agent._err()
    w[e, j, col] = was if dtype == "bf16" else next(c for c, v in E4M3.items() if v == was)
    # slot 131 + 70: expert 3's first row tile (row tile 3), rows 64.. (wr 1); another row of X
    s = 131 + 70
    ids[s] = (int(ids[s]) + 1) % TOKENS
    recs, _c = _run(agent, dtype, x, w, ids, offsets)
    assert bad(recs) == [4 * (3 * 2 + tj) + 2 * 1 + wc for tj in range(2) for wc in range(2)]


@pytest.mark.gpu
def test_gpu_unreferenced_nan_rows_and_hostile_indices_stay_in_bounds(agent):
    counts, n, k = COUNTS[5], 256, 128
    x, w, ids, offsets = _filled(agent, "bf16", counts, n, k)
    unused = sorted(set(range(TOKENS)) - set(ids.tolist()))
    assert unused  # 467 draws of 300 leave some rows unnamed
    x[unused] = float("nan")
    recs, c = _run(agent, "bf16", x, w, ids, offsets)
    assert np.array_equal(c, ref(SEED, counts, n, k, 1)[3])
    # row ids out of range, offsets below 0, beyond the slots and going down: the running
    # maximum of the clamped offsets ends at 260, so the rows from there on are nobody's
    x[unused] = 0.0
    ids[::7] = 10 ** 9
    ids[3::11] = -5
    offsets.copy_(torch.tensor([-7, 200, 100, 150, 260, 10 ** 9 - 2 ** 31], dtype=torch.int32))
    recs, c = _run(agent, "bf16", x, w, ids, offsets)
    assert np.isfinite(c).all() and (c[260:] == -1).all() and len(recs) == 4 * bound_of(counts, n)


@pytest.mark.gpu
def test_gpu_operation_against_float64(agent):
    """Random bf16 normals. The products of bf16 are exact in f32 and each of the
    K f32 additions of an element contributes at most one unit of 2^-23 of the
    sum of magnitudes (the MFMA's internal rounding is not documented: nearest
    is not assumed), so |C - exact| <= K 2^-23 (|X_g| |W_e|^T)."""
    counts, n, k = COUNTS[5], 512, 192
    gen = torch.Generator().manual_seed(20261126)
    x = torch.randn((TOKENS, k), generator=gen).bfloat16()
    w = torch.randn((len(counts), n, k), generator=gen).bfloat16()
    ids = torch.randint(0, TOKENS, (slots_of(counts),), generator=gen, dtype=torch.int32)
    offsets = torch.tensor([sum(counts[:e]) for e in range(len(counts) + 1)], dtype=torch.int32)
    _recs, c = _run(agent, "bf16", x.cuda(), w.cuda(), ids.cuda(), offsets.cuda())
    worst = 0.0
    for e in np.flatnonzero(counts):
        rows = slice(int(offsets[e]), int(offsets[e + 1]))
        xg, we = x[ids[rows].long()].double(), w[e].double()
        err = (torch.from_numpy(c[rows]).double() - xg @ we.T).abs()
        worst = max(worst, (err / (k * 2.0 ** -23 * (xg.abs() @ we.abs().T))).max().item())
    print("largest error over the bound K 2^-23 |X||W|^T:", worst)
    assert worst <= 1.0 and (c[sum(counts):] == -1).all()


@pytest.mark.gpu
def test_gpu_default_sweep_and_health_check(agent):
    torch.cuda.synchronize()
    res = agent.moe_gemm_sweep(0)
    _, _, _, cus = agent.device_info(0)
    print(f"moe_gemm_sweep: {res.tflops:.1f} TFLOP/s at {res.sweep.clock_mhz:.0f} MHz, "
          f"{res.sweep.units_seen} of {cus} CUs, {res.sweep.waves} records")
    assert res.ok, res.describe() + agent._err()
    assert res.sweep.waves == 4 * (32768 // 128 + 32) * 8 and res.sweep.units_seen == cus
    assert res.tflops >= nodeagent.MIN_MOE_GEMM_SWEEP_TFLOPS > 0
    g = agent.check(bw_bytes=1 << 28, moe_gemm_sweep=True).gpus[0]
    assert g.healthy, g.problems
    assert g.moe_gemm_sweep_tflops >= nodeagent.MIN_MOE_GEMM_SWEEP_TFLOPS
    assert g.moe_gemm_sweep_units_seen == g.cus and g.moe_gemm_sweep_clock_mhz > 0
    assert g.moe_gemm_sweep_bad_waves == 0 and g.moe_gemm_sweep_skipped == ""
