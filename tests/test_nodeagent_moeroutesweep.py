"""Chip-wide MoE routing sweep of the node agent (nodeagent/moeroutesweep.h):
the router (weights and top-k), the stable sort of (token, choice) pairs into
expert-major slots, and the weighted combine of the expert rows back into
token order.

The reference is the numpy copy of the specification below: keys from the bf16
bits, a stable argsort on (-key, index), float64 weights and sums, a stable
sort by expert, and every wave's checksum as the direct sum over its tokens. It
shares nothing with the host code's integer route or its factored combine. The
GPU tests change an element of their own tensors to see detection: a data
mismatch; nothing on the GPU is provoked.
"""
import ctypes
import functools
import json
import math

import numpy as np
import pytest

# torch first, before any test loads the agent library: see the note at the
# top of test_nodeagent_memtest.py (one HIP runtime per process -- torch's).
try:
    import torch
except ImportError:  # CPU-only environment: the GPU tests cannot run there
    torch = None

from gpu_provisioner_amd import nodeagent
from tests.test_nodeagent_gemmsweep import G, M64, U64, _ensure_lib
from tests.test_nodeagent_mfmasweep import FakeLib as MfmaFakeLib
from tests.test_nodeagent_mfmasweep import _mix64

SEED = getattr(nodeagent, "DEFAULT_MOE_ROUTE_SWEEP_SEED", 0)
N = 256
# a lone token with every expert chosen; both sides of the 256-token block edge; several
# blocks, so block_base matters; a row tail that is no multiple of 16; the maximum
SHAPES = [(1, 8, 8), (255, 16, 1), (256, 64, 2), (257, 80, 4), (1000, 256, 8), (1000, 80, 4)]
LOG2E = float(np.float32(math.log2(math.e)))


def route_ref(bits, top_k, scale, renorm):
    """(ids, p, denom, p of every expert, argument of every expert) of uint16 bf16 bits."""
    b = bits.astype(np.int64)
    nan = (b & 0x7FFF) > 0x7F80
    key = np.where(nan, 0, np.where(b & 0x8000 != 0, ~b & 0xFFFF, b | 0x8000))
    ids = np.argsort(-key, axis=1, kind="stable")[:, :top_k]
    with np.errstate(invalid="ignore", over="ignore"):
        x = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        m = np.where(nan.all(1), 0.0, np.where(nan, -np.inf, x).max(1))
        arg = scale * (x - m[:, None])
        p_all = np.where(nan, 0.0, np.exp2(arg))
    p = np.take_along_axis(p_all, ids, 1)
    return ids, p, (p if renorm else p_all).sum(1), p_all, arg


def sort_ref(ids, experts):
    """(offsets, row_ids, slot_of) of the stable sort by expert."""
    order = np.argsort(ids.ravel(), kind="stable")
    slot_of = np.empty(ids.size, dtype=np.int64)
    slot_of[order] = np.arange(ids.size)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(ids.ravel(), minlength=experts))])
    return offsets, order // ids.shape[1], slot_of.reshape(ids.shape)


@functools.lru_cache(maxsize=None)
def ref(seed, tokens, experts, top_k, renorm):
    """The hashed problem at N columns: (logit bits, ids, offsets, row_ids, slot_of, Y, checksums)."""
    slots = tokens * top_k
    with np.errstate(over="ignore"):
        def front(first, count):
            return _mix64(U64((seed * G + first) & M64) + np.arange(count, dtype=U64))

        def back(first, count):
            return _mix64(U64((seed * G - 1 - first) & M64) - np.arange(count, dtype=U64))

        def factors(x):
            return ((x >> U64(40)) % U64(3)).astype(np.int64) - 1, ((x >> U64(20)) % U64(3)).astype(np.int64) - 1

        logits = ((front(0, tokens) >> U64(40)) % U64(7)).astype(np.int64)[:, None] - 3 \
            - ((front(tokens, tokens * experts) >> U64(40)) % U64(9)).astype(np.int64).reshape(tokens, experts)
        bits = (logits.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        ids, p, denom, _, _ = route_ref(bits, top_k, 1.0, renorm)
        offsets, row_ids, slot_of = sort_ref(ids, experts)
        (a, b), (g, h) = factors(back(4 * slots + 2 * tokens, slots)), factors(back(5 * slots + 2 * tokens + N, N))
        y = a[:, None] * g[None, :] + b[:, None] * h[None, :]
        w_id, w_p, w_slot, w_row = (back(first, slots).reshape(tokens, top_k) | U64(1) for first in (
            0, slots, 2 * slots + tokens, 3 * slots + 2 * tokens))
        w_denom, w_token = back(2 * slots, tokens) | U64(1), back(3 * slots + tokens, tokens) | U64(1)
        q = back(5 * slots + 2 * tokens, N) | U64(1)
        p256 = (256 * p).astype(np.int64)
        sums = (p256[:, :, None] * y[slot_of]).sum(1)  # 256 * the combine's sum, exact
        per_token = [
            (w_id * ids.astype(U64) + w_p * p256.astype(U64)).sum(1) + w_denom * (256 * denom).astype(U64),
            (w_slot * (slot_of + 1).astype(U64)).sum(1),
            w_token * (q[None, :] * sums.astype(U64)).sum(1) + (w_row * (row_ids[slot_of] + 1).astype(U64)).sum(1)]
        route, scatter, combine = nodeagent.moe_route_records(tokens)
        want = []
        for part, per, count in zip(per_token, (64, 64, 8), (route, scatter, combine)):
            padded = np.zeros(count * per, dtype=U64)
            padded[:tokens] = part
            want += [int(v) for v in padded.reshape(count, per).sum(1, dtype=U64)]
    return bits, ids, offsets, row_ids, slot_of, y, want


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


@pytest.mark.parametrize("renorm", [0, 1])
@pytest.mark.parametrize("tokens,experts,top_k", SHAPES)
def test_expected_matches_direct_computation(cpu_agent, tokens, experts, top_k, renorm):
    assert cpu_agent.moe_route_expected(tokens, experts, top_k, N, renorm, SEED) \
        == ref(SEED, tokens, experts, top_k, renorm)[6]
    if tokens == 257:  # and a seed past 2^40, whose high half matters
        big = (1 << 40) + 9
        got = cpu_agent.moe_route_expected(tokens, experts, top_k, N, renorm, big)
        assert got == ref(big, tokens, experts, top_k, renorm)[6]
        assert got != cpu_agent.moe_route_expected(tokens, experts, top_k, N, renorm, big & 0xFFFFFFFF)


@pytest.mark.parametrize("tokens,experts,top_k,n,n_delta", [
    (300, 8, 0, 256, 0),         # no choice
    (300, 16, 9, 256, 0),        # more than 8 choices
    (300, 4, 5, 256, 0),         # more choices than experts
    (300, 257, 2, 256, 0),       # more than 256 experts
    (1 << 20, 8, 5, 256, 0),     # tokens * top_k over NA_MOE_MAX_ROWS
    (300, 8, 2, 258, 0),         # N no multiple of 4
    (300, 8, 2, 256, 4),         # a record buffer of the wrong size
])
def test_argument_errors_before_any_hip_call(cpu_agent, tokens, experts, top_k, n, n_delta):
    lib, bad, ptr = cpu_agent.lib, nodeagent.NA_ERR_ARG, 1 << 40  # the pointer is never followed
    route, scatter, combine = (count + n_delta for count in nodeagent.moe_route_records(tokens))
    size = route + scatter + combine - 2 * n_delta
    out, recs, res = (ctypes.c_uint64 * size)(), (nodeagent.MfmaRecord * size)(), nodeagent._MfmaSweepResultC()
    # a device that does not exist: the arguments are refused before it is looked at
    calls = {
        "na_moe_route_expected": lambda: lib.na_moe_route_expected(SEED, tokens, experts, top_k, n, 0, out, size),
        "na_moe_route_verify": lambda: lib.na_moe_route_verify(recs, size, tokens, experts, top_k, n, 0, SEED,
                                                               ctypes.byref(res)),
        "na_moe_route_run": lambda: lib.na_moe_route_run(99, ptr, ptr, ptr, ptr, tokens, experts, top_k, 1.0, 0,
                                                         SEED, recs, route, None),
        "na_moe_sort_run": lambda: lib.na_moe_sort_run(99, ptr, ptr, ptr, ptr, tokens, experts, top_k, SEED, recs,
                                                       scatter, None),
        "na_moe_combine_run": lambda: lib.na_moe_combine_run(99, ptr, ptr, ptr, ptr, ptr, ptr, tokens, top_k, n,
                                                             SEED, recs, combine, None),
        "na_moe_route_fill": lambda: lib.na_moe_route_fill(99, ptr, ptr, tokens, experts, top_k, n, SEED),
        "na_moe_route_sweep": lambda: lib.na_moe_route_sweep(99, tokens, experts, top_k, n, 1, SEED,
                                                             ctypes.byref(res), None, None),
    }
    if n % 4:  # the route and the sort do not know N
        del calls["na_moe_route_run"], calls["na_moe_sort_run"]
    if 1 <= top_k <= 8 and tokens * top_k <= 1 << 22 and n % 4 == 0 and not n_delta:
        del calls["na_moe_combine_run"]  # which does not know the experts
    if n_delta:  # neither the fill nor the whole sweep takes records
        del calls["na_moe_route_fill"], calls["na_moe_route_sweep"]
    if top_k == 0:  # 0 is the whole sweep's default
        del calls["na_moe_route_sweep"]
    for name, call in calls.items():
        assert call() == bad, name
        assert name in cpu_agent._err()


class FakeLib(MfmaFakeLib):
    """The matrix-core sweep's stand-in plus na_moe_route_sweep. ``moe``: {dev:
    "sick" | "slow" | "noroom"}; default clean."""

    def __init__(self, ngpu=1, moe=None):
        super().__init__(ngpu=ngpu)
        self.moe_calls = []

        def na_moe_route_sweep(dev, tokens, experts, top_k, n, reps, seed, res, mtoks, gbps):
            self.moe_calls.append((dev, tokens, experts, top_k, n, reps, seed))
            kind = (moe or {}).get(dev, "ok")
            if kind == "noroom":
                self.error = b"na_moe_route_sweep: the operands of 1392508928 bytes do not fit: 1 bytes"
                return nodeagent.NA_ERR_ARG
            r = res._obj
            r.waves, r.units_seen, r.clock_mhz = 10240, 256, 1801.26
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 0, 0, nodeagent.NO_BAD_WAVE, 0
            mtoks._obj.value, gbps._obj.value = (1.5, 2.5) if kind == "slow" else (901.26, 4001.26)
            if kind != "sick":
                return 0
            r.bad_waves, r.bad_units, r.first_bad_wave, r.listed = 1, 1, 1024 + 37, 1
            r.bad_list[0][:] = r.first_bad_unit[:] = (5, 2, 1, 9, 3)
            return nodeagent.NA_ERR_VERIFY

        self.na_moe_route_sweep = na_moe_route_sweep


def test_flag_reaches_check_through_the_cli(monkeypatch, capsys):
    monkeypatch.setattr(nodeagent, "MIN_MOE_ROUTE_SWEEP_MTOKS", 400.0)
    monkeypatch.setattr(nodeagent, "MIN_MOE_COMBINE_SWEEP_GBPS", 3000.0)
    fakes = []
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fakes[-1])
    fakes.append(FakeLib())
    assert nodeagent.main([]) == 0 and fakes[-1].moe_calls == []
    capsys.readouterr()
    assert nodeagent.main(["--moe-route-sweep"]) == 0
    assert fakes[-1].moe_calls == [(0, 0, 0, 0, 0, 0, SEED)] and fakes[-1].sweep_calls == []
    g = json.loads(capsys.readouterr().out)["gpus"][0]
    assert [g[f] for f in ("moe_route_sweep_mtoks", "moe_combine_sweep_gbps", "moe_route_sweep_clock_mhz",
                           "moe_route_sweep_units_seen", "moe_route_sweep_bad_waves",
                           "moe_route_sweep_skipped")] == [901.3, 4001.3, 1801.3, 256, 0, ""]
    fakes.append(FakeLib(ngpu=2, moe={1: "sick"}))
    report = nodeagent.NodeAgent().check(moe_route_sweep=True)
    assert report.problems == [
        "gpu1: MoE routing sweep: 1 of 10240 waves wrong on 1 CU(s): xcc5.se2.sh1.cu9 simd 3; first "
        "record 1061 (scatter, tokens 2368..2431) on xcc5.se2.sh1.cu9.simd3"]
    fakes.append(FakeLib(moe={0: "slow"}))
    assert nodeagent.NodeAgent().check(moe_route_sweep=True).gpus[0].problems == [
        "MoE routing sweep 1.5 Mtoken/s below floor 400.0", "MoE combine sweep 2.5 GB/s below floor 3000.0"]
    fakes.append(FakeLib(moe={0: "noroom"}))
    g = nodeagent.NodeAgent().check(moe_route_sweep=True).gpus[0]
    assert g.healthy and "do not fit" in g.moe_route_sweep_skipped and g.moe_route_sweep_mtoks == 0.0


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _layer(agent, logits, y, top_k, scale=1.0, renorm=0, change=None):
    """route -> sort -> combine on the GPU; ``y`` may be a function of (row_ids, offsets) that
    returns the rows, ``change(stage, tensors)`` edits the tensors between the kernels. Returns
    the tensors and the records of the three kernels, one behind the other."""
    tokens, experts = logits.shape
    def dev(shape, dtype):
        return torch.full(shape, -1, dtype=dtype, device="cuda:0")
    t = dict(ids=dev((tokens, top_k), torch.int32), p=dev((tokens, top_k), torch.float32),
             denom=dev((tokens,), torch.float32), offsets=dev((experts + 1,), torch.int32),
             row_ids=dev((tokens * top_k,), torch.int32), slot_of=dev((tokens, top_k), torch.int32))
    change = change or (lambda stage, tensors: None)
    torch.cuda.synchronize()
    recs = list(agent.moe_route_run(0, logits.data_ptr(), t["ids"].data_ptr(), t["p"].data_ptr(),
                                    t["denom"].data_ptr(), tokens, experts, top_k, scale, renorm, SEED)[0])
    change("routed", t)
    torch.cuda.synchronize()
    recs += agent.moe_sort_run(0, t["ids"].data_ptr(), t["offsets"].data_ptr(), t["row_ids"].data_ptr(),
                               t["slot_of"].data_ptr(), tokens, experts, top_k, SEED)[0]
    change("sorted", t)
    t["y"] = y(t["row_ids"], t["offsets"]) if callable(y) else y
    t["out"] = dev((tokens, t["y"].shape[1]), torch.float32)
    torch.cuda.synchronize()
    recs += agent.moe_combine_run(0, t["y"].data_ptr(), t["slot_of"].data_ptr(), t["row_ids"].data_ptr(),
                                  t["p"].data_ptr(), t["denom"].data_ptr(), t["out"].data_ptr(), tokens, top_k,
                                  t["y"].shape[1], SEED)[0]
    return {k: v.cpu().numpy() for k, v in t.items()}, (nodeagent.MfmaRecord * len(recs))(*recs)


def _hashed(agent, tokens, experts, top_k):
    logits = torch.empty((tokens, experts), dtype=torch.bfloat16, device="cuda:0")
    y = torch.empty((tokens * top_k, N), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    agent.moe_route_fill(0, logits.data_ptr(), y.data_ptr(), tokens, experts, top_k, N, SEED)
    return logits, y


@pytest.mark.gpu
@pytest.mark.parametrize("renorm", [0, 1])
@pytest.mark.parametrize("tokens,experts,top_k", SHAPES)
def test_gpu_every_record_and_index_is_exact(agent, tokens, experts, top_k, renorm):
    bits, ids, offsets, row_ids, slot_of, want_y, want = ref(SEED, tokens, experts, top_k, renorm)
    logits, y = _hashed(agent, tokens, experts, top_k)
    assert np.array_equal(logits.view(torch.int16).cpu().numpy().view(np.uint16), bits)
    assert np.array_equal(y.cpu().numpy(), want_y)
    got, recs = _layer(agent, logits, y, top_k, renorm=renorm)
    for name, array in (("ids", ids), ("offsets", offsets), ("row_ids", row_ids), ("slot_of", slot_of)):
        assert np.array_equal(got[name], array), name
    assert [r.checksum for r in recs] == want and [r.wave for r in recs] == list(range(len(want)))
    assert all(r.cycles > 0 and r.realtime > 0 for r in recs)
    rc, res = agent.moe_route_verify(recs, tokens, experts, top_k, N, renorm, SEED)
    assert rc == nodeagent.NA_OK and res.sweep.bad_waves == 0, agent._err()


def _p_bounds(p_all, arg, ids, renorm, experts):
    """The header's bounds of p (tokens x top_k) and denom, from float64 values."""
    with np.errstate(invalid="ignore"):
        each = p_all * (np.abs(np.where(p_all > 0, arg, 0.0)) * 2.0 ** -23 * math.log(2) + 2 * 2.0 ** -23) + 2.0 ** -126
    chosen = np.take_along_axis(each, ids, 1)
    terms, total = (chosen, ids.shape[1]) if renorm else (each, experts)
    return chosen, terms.sum(1) + total * 2.0 ** -24 * (np.take_along_axis(p_all, ids, 1) if renorm else p_all).sum(1)


def _random_logits(tokens, experts, gen):
    """Normal, deviation 4, with planted duplicates, an all-equal row, -inf, NaN and an all-NaN row."""
    logits = (4 * torch.randn((tokens, experts), generator=gen)).bfloat16()
    logits[:, experts // 2] = logits[:, 0]  # exact duplicates across experts, in every row
    logits[3 % tokens] = 1.5
    logits[::5, 1::3] = float("-inf")
    if tokens > 8:
        logits[7, ::2] = float("nan")
        logits[8] = float("nan")
    return logits


@pytest.mark.gpu
@pytest.mark.parametrize("tokens,experts,top_k,renorm", [(300, 16, 1, 0), (257, 64, 2, 1), (1000, 80, 4, 0),
                                                         (300, 256, 8, 1)])
def test_gpu_operation_against_float64(agent, tokens, experts, top_k, renorm):
    """Random logits under the natural softmax (scale log2 e). The indices are exact; p and denom
    are within the header's bounds of the float64 values; out is within (top_k + 2) roundings of
    the float64 combine of the device's own p and denom."""
    gen = torch.Generator().manual_seed(20261126)
    logits = _random_logits(tokens, experts, gen)
    y = torch.randn((tokens * top_k, N), generator=gen)
    got, _recs = _layer(agent, logits.cuda(), y.cuda(), top_k, LOG2E, renorm)
    ids, p, denom, p_all, arg = route_ref(logits.view(torch.int16).numpy().view(np.uint16), top_k, LOG2E, renorm)
    offsets, row_ids, slot_of = sort_ref(ids, experts)
    for name, array in (("ids", ids), ("offsets", offsets), ("row_ids", row_ids), ("slot_of", slot_of)):
        assert np.array_equal(got[name], array), name
    p_bound, denom_bound = _p_bounds(p_all, arg, ids, renorm, experts)
    worst_p = (np.abs(got["p"] - p) / p_bound).max()
    worst_denom = (np.abs(got["denom"] - denom) / denom_bound).max()
    rows = y.numpy().astype(np.float64)[slot_of] * got["p"].astype(np.float64)[:, :, None]
    ok = got["denom"] > 0  # the all-NaN row has weights 0 and denom 0: 0 * inf
    exact = rows.sum(1)[ok] / got["denom"].astype(np.float64)[ok, None]
    bound = (top_k + 2) * 2.0 ** -24 * (1 + 2.0 ** -20) * np.abs(rows).sum(1)[ok] / got["denom"][ok, None]
    worst_out = (np.abs(got["out"][ok] - exact) / np.maximum(bound, 1e-300)).max()
    print(f"largest error over its bound: p {worst_p:.3f}, denom {worst_denom:.3f}, out {worst_out:.3f}")
    assert worst_p <= 1.0 and worst_denom <= 1.0 and worst_out <= 1.0
    assert ok.sum() >= tokens - 1 and np.isnan(got["out"][~ok]).all()


@pytest.mark.gpu
def test_gpu_whole_layer_against_float64(agent):
    """Logits to output with no host step: route -> sort -> the expert GEMM on the sort's own
    row_ids and offsets -> combine, against a float64 layer from the logits. The bound is the sum of
    the kernels': K 2^-23 |x||W|^T of the GEMM (test_nodeagent_moegemmsweep.py) under the weights,
    the relative bounds of p and denom on the exact rows, and the combine's roundings; 2^-10 more of
    it covers the products of these first-order terms."""
    tokens, experts, top_k, k = 300, 5, 2, 64
    gen = torch.Generator().manual_seed(20261127)
    logits = _random_logits(tokens, experts, gen)
    x, w = torch.randn((tokens, k), generator=gen).bfloat16(), torch.randn((experts, N, k), generator=gen).bfloat16()
    x_dev, w_dev = x.cuda(), w.cuda()

    def gemm(row_ids, offsets):
        c = torch.zeros((tokens * top_k, N), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        agent.moe_gemm_run(0, x_dev.data_ptr(), w_dev.data_ptr(), row_ids.data_ptr(), offsets.data_ptr(), tokens,
                           tokens * top_k, experts, N, k, 1, SEED, "bf16", c.data_ptr())
        return c

    got, _recs = _layer(agent, logits.cuda(), gemm, top_k, LOG2E, 0)
    ids, p, denom, p_all, arg = route_ref(logits.view(torch.int16).numpy().view(np.uint16), top_k, LOG2E, 0)
    assert np.array_equal(got["ids"], ids)
    p_bound, denom_bound = _p_bounds(p_all, arg, ids, 0, experts)
    ok = denom > 0
    weight = (p[ok] / denom[ok, None])[:, :, None]
    relative = (p_bound[ok] / np.maximum(p[ok], 1e-300) + (denom_bound[ok] / denom[ok])[:, None])[:, :, None]
    xd, wd = x.double().numpy()[ok], w.double().numpy()[ids[ok]]  # (tokens, top_k, N, K)
    rows, sizes = np.einsum("tk,tjnk->tjn", xd, wd), np.einsum("tk,tjnk->tjn", np.abs(xd), np.abs(wd))
    bound = (weight * (k * 2.0 ** -23 * sizes + np.abs(rows) * relative)).sum(1) \
        + (top_k + 2) * 2.0 ** -24 * (weight * np.abs(rows)).sum(1)
    worst = (np.abs(got["out"][ok] - (weight * rows).sum(1)) / (bound * (1 + 2.0 ** -10))).max()
    print("largest error of the whole layer over the sum of the bounds:", worst)
    assert worst <= 1.0


@pytest.mark.gpu
def test_gpu_a_changed_id_or_slot_is_named(agent):
    tokens, experts, top_k = 1000, 80, 4
    _bits, ids, _offsets, _row_ids, slot_of, _y, _want = ref(SEED, tokens, experts, top_k, 0)
    logits, y = _hashed(agent, tokens, experts, top_k)
    route, scatter, _combine = nodeagent.moe_route_records(tokens)

    def another_expert(stage, t):  # token 500's third choice, to an expert it has not chosen
        if stage == "routed":
            t["ids"][500, 2] = next(e for e in range(experts) if e not in ids[500])

    _got, recs = _layer(agent, logits, y, top_k, change=another_expert)
    rc, res = agent.moe_route_verify(recs, tokens, experts, top_k, N, 0, SEED)
    assert rc == nodeagent.NA_ERR_VERIFY and route <= res.sweep.first_bad_wave < route + scatter
    assert "(scatter, tokens " in agent._err() and "scatter" in res.describe()

    def another_slot(stage, t):  # token 700 reads token 3's first row
        if stage == "sorted":
            t["slot_of"][700, 0] = int(slot_of[3, 0])

    _got, recs = _layer(agent, logits, y, top_k, change=another_slot)
    rc, res = agent.moe_route_verify(recs, tokens, experts, top_k, N, 0, SEED)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.sweep.bad_waves, res.sweep.first_bad_wave) == (1, route + scatter + 700 // 8)
    assert "(combine, tokens 696..703)" in agent._err() and "combine, tokens 696..703" in res.describe()


@pytest.mark.gpu
def test_gpu_default_sweep_and_health_check(agent):
    torch.cuda.synchronize()
    res = agent.moe_route_sweep(0)
    _, _, _, cus = agent.device_info(0)
    print(f"moe_route_sweep: {res.mtoks:.1f} Mtoken/s, combine {res.gbps:.1f} GB/s at "
          f"{res.sweep.clock_mhz:.0f} MHz, {res.sweep.units_seen} of {cus} CUs, {res.sweep.waves} records")
    assert res.ok, res.describe() + agent._err()
    assert res.sweep.waves == sum(nodeagent.moe_route_records(65536)) and res.sweep.units_seen == cus
    assert res.mtoks >= nodeagent.MIN_MOE_ROUTE_SWEEP_MTOKS > 0
    assert res.gbps >= nodeagent.MIN_MOE_COMBINE_SWEEP_GBPS > 0
    g = agent.check(bw_bytes=1 << 28, moe_route_sweep=True).gpus[0]
    assert g.healthy, g.problems
    assert g.moe_route_sweep_units_seen == g.cus and g.moe_route_sweep_clock_mhz > 0
    assert g.moe_route_sweep_bad_waves == 0 and g.moe_route_sweep_skipped == ""
