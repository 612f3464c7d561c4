"""Chip-wide fused attention sweep of the node agent (nodeagent/attnsweep.h):
bf16 flash attention with GQA and a bottom-right aligned causal mask.

The reference is the numpy copy of the specification below (``ref``): the
hashed integer tensors and dense integer attention, independent of the four
terms per pair the library's own expectation uses. The operation test holds
the kernel against torch float64 on the CPU. The attribution test flips one
element of its own tensor: a data mismatch; nothing on the GPU is provoked.
"""
import ctypes
import functools
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
from tests.test_nodeagent_gemmsweep import _ensure_lib
from tests.test_nodeagent_mfmasweep import _mix64

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
U64 = np.uint64
SEED = nodeagent.DEFAULT_ATTN_SWEEP_SEED
D = 128
# (heads, kv_heads, n_q, n_k, causal): one tile; odd tile count and GQA 2:1;
# diagonal tiles and two query blocks; an offset that is no multiple of 128
SHAPES = [(1, 1, 128, 64, 0), (2, 1, 128, 192, 0), (4, 2, 256, 256, 1), (1, 1, 128, 320, 1)]
CASES = [(*s, reps) for s in SHAPES for reps in (1, 3)]


def _hashed(first, count):
    with np.errstate(over="ignore"):
        return _mix64(U64(first & M64) + np.arange(count, dtype=U64))


@functools.lru_cache(maxsize=None)
def ref(seed, heads, kv_heads, n_q, n_k):
    """(Q, K, V, z, a, b, w) of the specification, the tensors as int64."""
    qbase = seed * G
    ubase = qbase + heads * n_q * 8
    ebase = ubase + kv_heads * D
    vbase = ebase + kv_heads * n_k * 4
    wbase = vbase + kv_heads * n_k * D
    bits = (_hashed(qbase, heads * n_q * 8) >> U64(40)).astype(np.int64)
    q = (bits[:, None] >> np.arange(16) & 1).reshape(heads, n_q, D) * 2 - 1
    u = ((_hashed(ubase, kv_heads * D) >> U64(40)) % U64(3)).astype(np.int64) - 1
    k = np.repeat(u.reshape(kv_heads, 1, D), n_k, axis=1)
    e = _hashed(ebase, kv_heads * n_k * 4).reshape(kv_heads, n_k, 4)
    column = 32 * np.arange(4) + (e >> U64(40) & U64(31)).astype(np.int64)
    value = 1 - 2 * (e >> U64(48) & U64(1)).astype(np.int64)
    hk, j, _ = np.indices(column.shape)
    k[hk, j, column] += value
    v = ((_hashed(vbase, kv_heads * n_k * D) >> U64(40)) % U64(3)).astype(np.int64) - 1
    weights = _hashed(wbase, 130 + heads * n_q) | U64(1)
    return (q, k, v.reshape(kv_heads, n_k, D), weights[:D], weights[D], weights[D + 1],
            weights[130:].reshape(heads, n_q))


@functools.lru_cache(maxsize=None)
def attention(seed, heads, kv_heads, n_q, n_k, causal):
    """(m, 256 l, 256 O) of one walk, exact integers: [heads][n_q]( [128])."""
    q, k, v, *_ = ref(seed, heads, kv_heads, n_q, n_k)
    group = heads // kv_heads
    s = np.einsum("hic,hjc->hij", q, np.repeat(k, group, axis=0))
    if causal:
        hidden = np.arange(n_k)[None, :] > np.arange(n_q)[:, None] + n_k - n_q
        s = np.where(hidden, -(1 << 20), s)
    m = s.max(axis=2)
    p = np.where(s - m[:, :, None] >= -8, 1 << np.maximum(8 + s - m[:, :, None], 0), 0)
    assert (p > 0).sum() == (s > -(1 << 19)).sum()  # s - m >= -8 for every visible pair
    return m, p.sum(axis=2), np.einsum("hij,hjc->hic", p, np.repeat(v, group, axis=0))


def checksums(seed, heads, kv_heads, n_q, n_k, causal, reps):
    *_, z, a, b, w = ref(seed, heads, kv_heads, n_q, n_k)
    m, l, o = attention(seed, heads, kv_heads, n_q, n_k, causal)
    with np.errstate(over="ignore"):
        row = U64(reps) * ((o.astype(U64) * z).sum(axis=2, dtype=U64) + a * l.astype(U64)) \
            + b * m.astype(U64)
        return [int(x) for x in (w * row).reshape(-1, 32).sum(axis=1, dtype=U64)]


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


@pytest.mark.parametrize("heads,kv_heads,n_q,n_k,causal,reps", CASES)
def test_expected_matches_the_dense_numpy_attention(cpu_agent, heads, kv_heads, n_q, n_k, causal,
                                                    reps):
    got = cpu_agent.attn_expected(heads, kv_heads, n_q, n_k, bool(causal), reps, SEED)
    assert got == checksums(SEED, heads, kv_heads, n_q, n_k, causal, reps)


@pytest.mark.parametrize("heads,kv_heads,n_q,n_k,causal,reps", [
    (1, 1, 128, 96, 0, 1),     # n_k no multiple of 64
    (1, 1, 256, 128, 1, 1),    # causal with n_k < n_q
    (3, 2, 128, 64, 0, 1),     # heads no multiple of kv_heads
    (1, 1, 128, 64, 0, 1024),  # 256 * reps * n_k = 2^24: beyond NA_ATTN_EXACT
    (1, 1, 64, 64, 0, 1),      # decode-sized n_q
])
def test_argument_errors_before_any_hip_call(cpu_agent, heads, kv_heads, n_q, n_k, causal, reps):
    n = max(heads * (n_q // 128) * 4, 1)
    out, recs = (ctypes.c_uint64 * n)(), (nodeagent.MfmaRecord * n)()
    lib = cpu_agent.lib
    assert lib.na_attn_sweep_expected(SEED, heads, kv_heads, n_q, n_k, causal, reps, out,
                                      n) == nodeagent.NA_ERR_ARG
    # a device that does not exist: the shape is refused before it is looked at
    assert lib.na_attn_run(99, 16, 16, 16, None, heads, kv_heads, n_q, n_k, causal, 1.0, reps,
                           SEED, recs, n, None) == nodeagent.NA_ERR_ARG
    rc, _res = cpu_agent.attn_verify(recs, heads, kv_heads, n_q, n_k, bool(causal), reps, SEED)
    assert rc == nodeagent.NA_ERR_ARG


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _filled(agent, heads, kv_heads, n_q, n_k):
    q = torch.empty((heads, n_q, D), dtype=torch.bfloat16, device="cuda:0")
    k = torch.empty((kv_heads, n_k, D), dtype=torch.bfloat16, device="cuda:0")
    v = torch.empty_like(k)
    torch.cuda.synchronize()
    agent.attn_fill(0, q.data_ptr(), k.data_ptr(), v.data_ptr(), heads, kv_heads, n_q, n_k, SEED)
    return q, k, v


def _run(agent, q, k, v, causal, scale, reps=1):
    heads, n_q, _ = q.shape
    o = torch.full((heads, n_q, D), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    recs, _ms = agent.attn_run(0, q.data_ptr(), k.data_ptr(), v.data_ptr(), heads, k.shape[0], n_q,
                               k.shape[1], bool(causal), scale, reps, SEED, o.data_ptr())
    return recs, o.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("heads,kv_heads,n_q,n_k,causal,reps", CASES)
def test_gpu_every_wave_is_exact(agent, heads, kv_heads, n_q, n_k, causal, reps):
    q, k, v = _filled(agent, heads, kv_heads, n_q, n_k)
    for got, want in zip((q, k, v), ref(SEED, heads, kv_heads, n_q, n_k)):
        assert np.array_equal(got.float().cpu().numpy(), want)
    recs, o = _run(agent, q, k, v, causal, math.log(2), reps)  # scale_log2 = 1
    want = checksums(SEED, heads, kv_heads, n_q, n_k, causal, reps)
    rc, res = agent.attn_verify(recs, heads, kv_heads, n_q, n_k, bool(causal), reps, SEED)
    assert (rc, res.sweep.bad_waves, res.sweep.waves) == (nodeagent.NA_OK, 0, len(want))
    assert [r.checksum for r in recs] == want
    if reps == 1:
        # O and l are exact, so only the final division rounds: 1 ulp of f32
        _m, l, o256 = attention(SEED, heads, kv_heads, n_q, n_k, causal)
        exact = o256 / l[:, :, None].astype(np.float64)
        err = np.abs(o - exact) / np.spacing(np.abs(exact).astype(np.float32))
        print("largest error in ulp:", err.max())
        assert err.max() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("heads,kv_heads,n_q,n_k,causal", SHAPES)
def test_gpu_operation_against_float64(agent, heads, kv_heads, n_q, n_k, causal):
    """Normal bf16 q and k of deviation 2, so that logits at the natural scale
    128^-1/2 have deviation about 4, and v uniform in [-1, 1]. P rounded to bf16
    contributes at most 2 * 2^-9 * max|v| (a relative 2^-9 in every weight, in
    numerator and in the f32 denominator's favour), the rest is f32; the bound
    is twice that."""
    gen = torch.Generator().manual_seed(20261126)
    q = (2 * torch.randn((heads, n_q, D), generator=gen)).bfloat16()
    k = (2 * torch.randn((kv_heads, n_k, D), generator=gen)).bfloat16()
    v = (2 * torch.rand((kv_heads, n_k, D), generator=gen) - 1).bfloat16()
    _recs, o = _run(agent, q.cuda(), k.cuda(), v.cuda(), causal, D ** -0.5)
    group = heads // kv_heads
    s = torch.einsum("hic,hjc->hij", q.double(), k.double().repeat_interleave(group, 0)) / D ** 0.5
    if causal:
        s = s.masked_fill(torch.ones(n_q, n_k).triu(n_k - n_q + 1).bool(), -math.inf)
    want = torch.softmax(s, dim=2) @ v.double().repeat_interleave(group, 0)
    atol = 2.0 ** -7 * v.abs().max().item()
    err = np.abs(o - want.numpy()).max()
    print("logit deviation", s[s > -math.inf].std().item(), "largest error", err, "atol", atol)
    assert err <= atol


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [0, 1])
def test_gpu_a_flipped_query_element_is_pinned_on_the_wave_that_owns_the_row(agent, causal):
    heads, kv_heads, n_q, n_k = 4, 2, 256, 256
    q, k, v = _filled(agent, heads, kv_heads, n_q, n_k)
    h, row = 3, 170  # head 3, block 1, wave 1: record 4 * (3 * 2 + 1) + 1
    # a column where the common mode u is not zero: the row maximum moves
    column = int(np.flatnonzero(ref(SEED, heads, kv_heads, n_q, n_k)[1][1].sum(axis=0) > n_k // 2)[0])
    q[h, row, column] = -q[h, row, column]
    recs, _o = _run(agent, q, k, v, causal, math.log(2))
    want = checksums(SEED, heads, kv_heads, n_q, n_k, causal, 1)
    assert [i for i, r in enumerate(recs) if r.checksum != want[i]] == [29]
    rc, res = agent.attn_verify(recs, heads, kv_heads, n_q, n_k, bool(causal), 1, SEED)
    assert (rc, res.sweep.bad_waves, res.sweep.first_bad_wave) == (nodeagent.NA_ERR_VERIFY, 1, 29)
    assert "head 3 rows 160..191" in agent._err() and "head 3 rows 160..191" in res.describe()


@pytest.mark.gpu
def test_gpu_sweep_and_health_check(agent):
    torch.cuda.synchronize()
    for causal in (False, True):
        res = agent.attn_sweep(0, heads=8, kv_heads=2, n_q=256, n_k=384, causal=causal, reps=2)
        assert res.ok and res.sweep.bad_waves == 0 and res.sweep.waves == 64
        assert res.sweep.units_seen >= 1 and res.tflops > 0
    g = agent.check(bw_bytes=1 << 28, attn_sweep=True).gpus[0]
    print("attention sweep:", g.attn_sweep_tflops, g.attn_sweep_causal_tflops, "TFLOP/s at",
          g.attn_sweep_clock_mhz, "MHz on", g.attn_sweep_units_seen, "CUs")
    assert g.attn_sweep_bad_waves == 0 and g.attn_sweep_units_seen >= 1, g.problems
    assert g.attn_sweep_tflops > 0 and g.attn_sweep_causal_tflops > 0 and g.attn_sweep_clock_mhz > 0
    assert not [p for p in g.problems if "attention" in p]
