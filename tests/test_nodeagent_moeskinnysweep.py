"""Chip-wide decode-size MoE expert GEMM sweep of the node agent
(nodeagent/moeskinnysweep.h): the MoE GEMM sweep's operation on the same tensors
in tiles of 16 slots x 256 columns, wave w on columns 64 w.. of its tile, tiles
numbered by expert, column tile, row tile.

The reference is test_nodeagent_moegemmsweep's numpy copy of the operation (its
exact C); the per-wave sums in this kernel's numbering are recomputed here as
direct sums. The GPU tests change an element of their own tensors to see
detection: a data mismatch; nothing on the GPU is provoked.
"""
import ctypes
import json

import numpy as np
import pytest

try:  # torch first: see the note at the top of test_nodeagent_memtest.py
    import torch
except ImportError:  # CPU-only environment: the GPU tests cannot run there
    torch = None

from gpu_provisioner_amd import nodeagent
from tests.test_nodeagent_gemmsweep import BK, E4M3, G, M64, U64, _values
from tests.test_nodeagent_moegemmsweep import TOKENS, FakeLib, _ensure_lib, _mix64, ref, slots_of

SEED = getattr(nodeagent, "DEFAULT_MOE_SKINNY_SWEEP_SEED", 0)
# one full tile; a single slot; one short of a tile; a second tile of one row; empty
# experts at both ends; no tile at all; a mixed set with three row tiles; more tiles
# than 8 XCDs and the wrap of the block map
COUNTS = [(16,), (1,), (15,), (17,), (0, 5, 0), (0, 0), (33, 0, 1, 16, 7),
          tuple(1 + 37 * i % 23 for i in range(20))]
MIXED = COUNTS[6]


def bound_of(counts, n):
    return (slots_of(counts) // 16 + len(counts)) * (n // 256)


def sums_of(seed, counts, n, k, reps):
    """Every record's checksum, from ref's exact C: 16 rows, 64 columns a wave."""
    c, slots, first = ref(seed, counts, n, k, reps)[3], slots_of(counts), TOKENS * k + len(counts) * n * k
    with np.errstate(over="ignore"):
        p = _mix64(U64((seed * G + first) & M64) + np.arange(slots, dtype=U64)) | U64(1)
        q = _mix64(U64((seed * G + first + slots) & M64) + np.arange(n, dtype=U64)) | U64(1)
        sums, s0 = [], 0
        for cnt in counts:
            for col in range(0, n, 256):
                for r0 in range(s0, s0 + cnt, 16):
                    rows = slice(r0, min(r0 + 16, s0 + cnt))
                    for cols in (slice(col + 64 * w, col + 64 * w + 64) for w in range(4)):
                        part = p[rows, None] * q[None, cols] * c[rows, cols].astype(np.int64).astype(U64)
                        sums.append(int(part.sum(dtype=U64)))
            s0 += cnt
    return sums + [0] * (4 * bound_of(counts, n) - len(sums))


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
    assert cpu_agent.moe_skinny_tiles(slots, len(counts), n) == bound_of(counts, n)
    assert cpu_agent.moe_skinny_expected(TOKENS, slots, n, k, counts, reps, SEED) \
        == sums_of(SEED, counts, n, k, reps)


@pytest.mark.parametrize("tokens,slots,counts,n,k,reps,n_delta", [
    (0, 8, (5,), 256, 64, 1, 0),          # no tokens
    (300, 0, (0,), 256, 64, 1, 0),        # no slots
    (300, 8, (5,) * 257, 256, 64, 1, 0),  # more than 256 experts
    (300, 8, (5,), 384, 64, 1, 0),        # N no multiple of 256
    (300, 8, (5,), 256, 96, 1, 0),        # K no multiple of 64
    (300, 8, (5,), 256, 8192, 342, 0),    # 6 * reps * K = 2^24 and more
    (300, 8, (5, 4), 256, 64, 1, 0),      # counts beyond the slots
    (300, 8, (5,), 256, 64, 1, 4),        # a record buffer of the wrong size
])
def test_argument_errors_before_any_hip_call(cpu_agent, tokens, slots, counts, n, k, reps, n_delta):
    lib, experts, bad = cpu_agent.lib, len(counts), nodeagent.NA_ERR_ARG
    size = 4 * (max(slots, 1) // 16 + experts) * max(n // 256, 1) + n_delta
    out, recs, res = (ctypes.c_uint64 * size)(), (nodeagent.MfmaRecord * size)(), nodeagent._MfmaSweepResultC()
    cnts, ptr = (ctypes.c_int * experts)(*counts), 1 << 40  # the pointer is never followed
    assert lib.na_moe_skinny_expected(SEED, tokens, slots, experts, n, k, cnts, reps, out, size) == bad
    assert "na_moe_skinny_expected" in cpu_agent._err()
    assert lib.na_moe_skinny_verify(recs, size, tokens, slots, experts, n, k, cnts, reps, SEED,
                                    ctypes.byref(res)) == bad
    assert "na_moe_skinny_verify" in cpu_agent._err()
    if sum(counts) <= slots:  # the run sees the counts on the device only; device 99 does not exist
        assert lib.na_moe_skinny_run(99, 0, ptr, ptr, ptr, ptr, None, tokens, slots, experts, n, k,
                                     reps, SEED, recs, size, None) == bad
        assert "na_moe_skinny_run" in cpu_agent._err()
    if n_delta:  # everything else is in order: the pointers and the dtype are looked at
        for args in [(0, ptr + 8, ptr, ptr, ptr, None), (0, ptr, ptr, ptr + 2, ptr, None),
                     (0, ptr, ptr, ptr, ptr, ptr + 4), (2, ptr, ptr, ptr, ptr, None)]:
            assert lib.na_moe_skinny_run(99, *args, tokens, slots, experts, n, k, reps, SEED, recs,
                                         size - n_delta, None) == bad, args
        assert lib.na_moe_skinny_sweep(99, 0, 0, 0, 257, 0, 0, 0, SEED, ctypes.byref(res), None) == bad
        assert lib.na_moe_skinny_tiles(slots, experts, n, None) == bad


def test_verify_names_the_wave_and_wants_the_surplus_idle(cpu_agent):
    n, k, slots, want = 512, 128, slots_of(MIXED), sums_of(SEED, MIXED, 512, 128, 2)
    recs = (nodeagent.MfmaRecord * len(want))()
    for i, r in enumerate(recs):
        r.checksum, r.wave, r.cycles, r.realtime = want[i], i, 21000, 1000
        r.xcc, r.se, r.sh, r.cu, r.simd = i // 4 % 8, i // 32 % 4, 0, i // 4 % 16, i % 4
    rc, res = cpu_agent.moe_skinny_verify(recs, TOKENS, slots, n, k, MIXED, 2, SEED)
    assert rc == nodeagent.NA_OK and res.ok and res.sweep.waves == 4 * bound_of(MIXED, n)
    # row tiles 3 + 0 + 1 + 1 + 1, two column tiles: tile 4 is expert 0's column tile 1,
    # row tile 1; tile 12 is the first idle one
    for wave, where in [(4 * 4 + 2, "expert 0 row tile 1 column tile 1 wave 2"),
                        (48, "a surplus workgroup that must report idle")]:
        recs[wave].checksum ^= 1 << 17
        rc, res = cpu_agent.moe_skinny_verify(recs, TOKENS, slots, n, k, MIXED, 2, SEED)
        recs[wave].checksum ^= 1 << 17
        assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
        assert (res.sweep.bad_waves, res.sweep.first_bad_wave) == (1, wave)
        unit = f"xcc{recs[wave].xcc}.se{recs[wave].se}.sh0.cu{recs[wave].cu}.simd{wave % 4}"
        assert f"first record {wave} ({where}) on {unit}" in cpu_agent._err()
        assert where.split(" wave")[0] in res.describe() and unit in res.describe()


class SkinnyFakeLib(FakeLib):
    """The MoE GEMM sweep's stand-in plus na_moe_skinny_sweep; ``slow``: its rate."""

    def __init__(self, slow=False):
        super().__init__()
        self.skinny_calls = []

        def na_moe_skinny_sweep(dev, dtype, tokens, slots, experts, n, k, reps, seed, res, gbps):
            self.skinny_calls.append((dev, dtype, tokens, slots, experts, n, k, reps, seed))
            r = res._obj
            r.waves, r.units_seen, r.clock_mhz = 6656, 256, 1801.26
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            gbps._obj.value = 1.5 if slow else 4001.26
            return 0

        self.na_moe_skinny_sweep = na_moe_skinny_sweep


def test_flag_reaches_check_through_the_cli(monkeypatch, capsys):
    monkeypatch.setattr(nodeagent, "MIN_MOE_SKINNY_SWEEP_GBPS", 3000.0)
    fakes = [SkinnyFakeLib()]
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fakes[-1])
    assert nodeagent.main([]) == 0 and fakes[-1].skinny_calls == []
    capsys.readouterr()
    assert nodeagent.main(["--moe-skinny-sweep"]) == 0
    assert fakes[-1].skinny_calls == [(0, 0, 0, 0, 0, 0, 0, 0, SEED)] and fakes[-1].moe_calls == []
    g = json.loads(capsys.readouterr().out)["gpus"][0]
    assert [g[f"moe_skinny_sweep_{f}"] for f in ("gbps", "clock_mhz", "units_seen", "bad_waves",
                                                 "skipped")] == [4001.3, 1801.3, 256, 0, ""]
    fakes.append(SkinnyFakeLib(slow=True))
    assert nodeagent.NodeAgent().check(moe_skinny_sweep=True).gpus[0].problems == [
        "MoE skinny sweep 1.5 GB/s below floor 3000.0"]


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _filled(agent, dtype, counts, n, k):
    """(X, W, row_ids, offsets) of na_moe_gemm_fill on the GPU."""
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
    recs, _ms = agent.moe_skinny_run(0, x.data_ptr(), w.data_ptr(), ids.data_ptr(), offsets.data_ptr(),
                                     x.shape[0], len(ids), w.shape[0], w.shape[1], x.shape[1], reps,
                                     SEED, dtype, c.data_ptr())
    return recs, c.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("counts,ksteps", [(counts, 3) for counts in COUNTS] + [(MIXED, 1)])
def test_gpu_every_record_and_c_are_exact(agent, counts, ksteps, dtype):
    n, k, reps = 512, ksteps * BK[dtype], 3
    x, w, ids, offsets = _filled(agent, dtype, counts, n, k)
    recs, c = _run(agent, dtype, x, w, ids, offsets, reps)
    assert np.array_equal(c, ref(SEED, counts, n, k, reps)[3])  # rows nobody owns keep their -1
    assert [r.checksum for r in recs] == sums_of(SEED, counts, n, k, reps)
    assert [r.wave for r in recs] == list(range(4 * bound_of(counts, n)))  # idle ones too
    rc, res = agent.moe_skinny_verify(recs, TOKENS, len(ids), n, k, counts, reps, SEED, dtype)
    assert rc == nodeagent.NA_OK and res.sweep.bad_waves == 0, agent._err()
    assert all(r.cycles > 0 and r.realtime > 0 for r in recs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_gpu_a_changed_weight_or_row_id_fails_exactly_the_waves_that_read_it(agent, dtype):
    n, k = 512, 2 * BK[dtype]
    x, w, ids, offsets = _filled(agent, dtype, MIXED, n, k)
    want = sums_of(SEED, MIXED, n, k, 1)

    def bad(recs):
        return [i for i, r in enumerate(recs) if r.checksum != want[i]]

    # W[0][400]: expert 0 is tiles 0..5, column tile 1 its tiles 3, 4, 5; column 400 is wave 2
    e, j, col = 0, 400, BK[dtype] + 17
    was = int(_values(w[e, j:j + 1, col:col + 1], dtype)[0, 0])
    now = 1 if was != 1 else 2  # another small integer, exact in both formats
    w[e, j, col] = now if dtype == "bf16" else next(c for c, v in E4M3.items() if v == now)
    assert bad(_run(agent, dtype, x, w, ids, offsets)[0]) == [4 * t + 2 for t in (3, 4, 5)]
    w[e, j, col] = was if dtype == "bf16" else next(c for c, v in E4M3.items() if v == was)
    # slot 39 is expert 3's (slots 34..49, one row tile): tile 8 and, in column tile 1, tile 9
    ids[39] = (int(ids[39]) + 1) % TOKENS
    assert bad(_run(agent, dtype, x, w, ids, offsets)[0]) == list(range(4 * 8, 4 * 10))


@pytest.mark.gpu
def test_gpu_unreferenced_nan_rows_and_hostile_indices_stay_in_bounds(agent):
    n, k = 256, 128
    x, w, ids, offsets = _filled(agent, "bf16", MIXED, n, k)
    want_x, want_w, _ids, want_c, _sums = ref(SEED, MIXED, n, k, 1)
    unused = sorted(set(range(TOKENS)) - set(ids.tolist()))
    assert unused  # 60 draws of 300 leave rows unnamed
    x[unused] = float("nan")
    assert np.array_equal(_run(agent, "bf16", x, w, ids, offsets)[1], want_c)
    # The kernel's clamps (moeskinnysweep.h, "Safety"): row ids to [0, tokens), offsets to
    # [0, slots] and then their running maximum: expert 0 is slots 0..19, expert 3 slots
    # 20..39, the others empty, the rows from 40 on nobody's.
    x, w, ids, offsets = _filled(agent, "bf16", MIXED, n, k)  # X without the NaN again
    ids[::7] = 10 ** 9
    ids[3::11] = -5
    offsets.copy_(torch.tensor([-7, 20, 10, 15, 40, 10 ** 9 - 2 ** 31], dtype=torch.int32))
    rows = np.clip(ids.cpu().numpy(), 0, TOKENS - 1)
    want = np.full_like(want_c, -1.0)
    for e, s in ((0, slice(0, 20)), (3, slice(20, 40))):
        want[s] = want_x[rows[s]].astype(np.float64) @ want_w[e].T.astype(np.float64)
    recs, c = _run(agent, "bf16", x, w, ids, offsets)
    assert np.array_equal(c, want) and len(recs) == 4 * bound_of(MIXED, n)


@pytest.mark.gpu
def test_gpu_operation_against_float64(agent):
    """Random bf16 normals; the MoE GEMM sweep's bound, which holds for any
    summation order: |C - exact| <= K 2^-23 (|X_g| |W_e|^T). Largest fraction of
    it observed on MI355X: see docs/DESIGN.md."""
    counts, n, k = (3, 0, 16, 21), 256, 256
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
    res = agent.moe_skinny_sweep(0)
    _, _, _, cus = agent.device_info(0)
    print(f"moe_skinny_sweep: {res.gbps:.1f} GB/s at {res.sweep.clock_mhz:.0f} MHz, "
          f"{res.sweep.units_seen} of {cus} CUs, {res.sweep.waves} records")
    assert res.ok, res.describe() + agent._err()
    assert res.sweep.waves == 4 * (1280 // 16 + 128) * 8 and res.sweep.units_seen == cus
    assert res.gbps >= nodeagent.MIN_MOE_SKINNY_SWEEP_GBPS > 0
    g = agent.check(bw_bytes=1 << 28, moe_skinny_sweep=True).gpus[0]
    assert g.healthy, g.problems
    assert g.moe_skinny_sweep_gbps >= nodeagent.MIN_MOE_SKINNY_SWEEP_GBPS
    assert g.moe_skinny_sweep_units_seen == g.cus and g.moe_skinny_sweep_clock_mhz > 0
    assert g.moe_skinny_sweep_bad_waves == 0 and g.moe_skinny_sweep_skipped == ""
