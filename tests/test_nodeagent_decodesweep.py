"""Chip-wide paged decode attention sweep of the node agent
(nodeagent/decodesweep.h): one bf16 query token per sequence against a KV cache
in pages of 16 tokens, GQA, the walk split over waves and workgroups.

The reference is the attention sweep's numpy specification (``ref`` of
test_nodeagent_attnsweep.py, under the mapping of decodesweep.h) and a dense
integer decode that cuts each row at its length and partitions the keys by
split and wave, independent of the four terms per pair the library's own
expectation uses. The operation test holds the kernel against torch float64 on
the CPU. The attribution test flips one element of its own tensor: a data
mismatch; nothing on the GPU is provoked.
"""
import ctypes
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
from tests.test_nodeagent_attnsweep import D, U64, ref
from tests.test_nodeagent_gemmsweep import _ensure_lib

SEED = nodeagent.DEFAULT_DECODE_SWEEP_SEED
PAGE, TILE = 16, 32
# (batch, heads, kv_heads, lens, splits): one key, three empty waves, 15 padded
# rows and a tile without its second page; a length one slot into a page, odd
# page counts, group 4, two rounds of the waves; a full group of 16 and splits
# the short sequences leave empty; group 3 and uneven split ranges
SHAPES = [(1, 1, 1, (1,), 1), (2, 8, 2, (17, 130), 1), (3, 16, 1, (300, 33, 64), 3),
          (2, 6, 2, (513, 128), 2)]
CASES = [(*s, reps) for s in SHAPES for reps in (1, 3)]
ARGS = "batch,heads,kv_heads,lens,splits"


def max_pages_of(lens):
    return -(-max(lens) // PAGE) + 1  # one table entry nobody may use


def spec(batch, heads, kv_heads, lens):
    """(q, k, v, z, a, b, w) of the specification as [batch][heads or kv_heads]..."""
    n_k = PAGE * max_pages_of(lens)
    q, k, v, z, a, b, w = ref(SEED, batch * heads, batch * kv_heads, 1, n_k)
    return (q.reshape(batch, heads, D), k.reshape(batch, kv_heads, n_k, D),
            v.reshape(batch, kv_heads, n_k, D), z, a, b, w.reshape(batch, heads))


def part_of(j, length, splits):
    """(split, wave) that owns key j of a sequence of `length` keys."""
    t, tiles = j // TILE, -(-length // TILE)
    s = next(s for s in range(splits) if s * tiles // splits <= t < (s + 1) * tiles // splits)
    return s, (t - s * tiles // splits) % 4


def decode(batch, heads, kv_heads, lens, splits):
    """{record index: [(head weight, m, 256 l, 256 O[128])]} of one walk and the
    exact output [batch][heads][128], by dense integer attention."""
    q, k, v, *_rest, w = spec(batch, heads, kv_heads, lens)
    group, finals = heads // kv_heads, 4 * batch * kv_heads * splits
    states, out = {}, np.zeros((batch, heads, D))
    for b, length in enumerate(lens):
        owner = np.array([part_of(j, length, splits) for j in range(length)])
        for h in range(heads):
            item = b * kv_heads + h // group
            s = k[b, h // group, :length] @ q[b, h]
            parts = [(finals + item, np.ones(length, bool))] + [
                (4 * (item * splits + sp) + wv, (owner == (sp, wv)).all(axis=1))
                for sp in range(splits) for wv in range(4)]
            for index, keys in parts:
                if not keys.any():
                    continue
                m = s[keys].max()
                assert (s[keys] - m).min() >= -8
                p = 1 << (8 + s[keys] - m)
                state = (w[b, h], m, p.sum(), p @ v[b, h // group, :length][keys])
                states.setdefault(index, []).append(state)
                if index >= finals:
                    out[b, h] = state[3] / state[2]
    return states, out


def checksums(batch, heads, kv_heads, lens, splits, reps):
    *_, z, a, b, _w = spec(batch, heads, kv_heads, lens)
    states, _out = decode(batch, heads, kv_heads, lens, splits)
    want = [0] * (batch * kv_heads * (4 * splits + 1))
    with np.errstate(over="ignore"):
        for index, rows in states.items():
            want[index] = int(sum(
                (w * (U64(reps) * ((o.astype(U64) * z).sum(dtype=U64) + a * U64(l))
                      + b * np.int64(m).astype(U64)) for w, m, l, o in rows), U64(0)))
    return want


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


@pytest.mark.parametrize(ARGS + ",reps", CASES)
def test_expected_matches_the_dense_numpy_decode(cpu_agent, batch, heads, kv_heads, lens, splits,
                                                 reps):
    got = cpu_agent.decode_expected(batch, heads, kv_heads, max_pages_of(lens), lens, splits,
                                    reps, SEED)
    assert got == checksums(batch, heads, kv_heads, lens, splits, reps)


@pytest.mark.parametrize("heads,kv_heads,max_pages,length,reps,n_delta", [
    (17, 1, 4, 8, 1, 0),      # group > 16
    (3, 2, 4, 8, 1, 0),       # heads no multiple of kv_heads
    (2, 1, 4, 0, 1, 0),       # a length of 0
    (2, 1, 4, 65, 1, 0),      # a length beyond 16 * max_pages
    (2, 1, 4, 64, 1024, 0),   # 256 * reps * len = 2^24: beyond NA_DECODE_EXACT
    (2, 1, 4, 8, 1, 1),       # a record buffer of the wrong size
])
def test_argument_errors_before_any_hip_call(cpu_agent, heads, kv_heads, max_pages, length, reps,
                                             n_delta):
    n = max(kv_heads, 1) * 5 + n_delta
    out, recs = (ctypes.c_uint64 * n)(), (nodeagent.MfmaRecord * n)()
    lens, lib = (ctypes.c_int * 1)(length), cpu_agent.lib
    assert lib.na_decode_sweep_expected(SEED, 1, heads, kv_heads, max_pages, lens, 1, reps, out,
                                        n) == nodeagent.NA_ERR_ARG
    assert lib.na_decode_sweep_verify(recs, n, 1, heads, kv_heads, max_pages, lens, 1, reps, SEED,
                                      ctypes.byref(nodeagent._MfmaSweepResultC())
                                      ) == nodeagent.NA_ERR_ARG
    # a device that does not exist: the arguments are refused before it is looked at
    if reps == 1 and not n_delta:  # the fill takes neither repetitions nor records
        assert lib.na_decode_sweep_fill(99, 16, 16, 16, 16, 16, 1, heads, kv_heads, max_pages,
                                        lens, SEED) == nodeagent.NA_ERR_ARG
    if length == 8:  # the run sees the lengths on the device only
        assert lib.na_decode_run(99, 16, 16, 16, 16, 16, None, 1, heads, kv_heads, max_pages, 5, 1,
                                 1.0, reps, SEED, recs, n, None) == nodeagent.NA_ERR_ARG


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _filled(agent, batch, heads, kv_heads, lens):
    """(q, k_cache, v_cache, block_table, seq_lens) of the sweep on the GPU."""
    max_pages = max_pages_of(lens)
    q = torch.empty((batch, heads, D), dtype=torch.bfloat16, device="cuda:0")
    kc = torch.empty((batch * max_pages + 1, kv_heads, PAGE, D), dtype=torch.bfloat16,
                     device="cuda:0")
    vc = torch.empty_like(kc)
    table = torch.empty((batch, max_pages), dtype=torch.int32, device="cuda:0")
    dlens = torch.empty((batch,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    agent.decode_fill(0, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), table.data_ptr(),
                      dlens.data_ptr(), batch, heads, kv_heads, max_pages, lens, SEED)
    return q, kc, vc, table, dlens


def _run(agent, q, kc, vc, table, dlens, splits, scale, reps=1):
    batch, heads, _ = q.shape
    o = torch.full((batch, heads, D), float("nan"), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    recs, _ms = agent.decode_run(0, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), table.data_ptr(),
                                 dlens.data_ptr(), batch, heads, kc.shape[1], table.shape[1],
                                 kc.shape[0], splits, scale, reps, SEED, o.data_ptr())
    return recs, o.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize(ARGS + ",reps", CASES)
def test_gpu_every_record_is_exact(agent, batch, heads, kv_heads, lens, splits, reps):
    tensors = _filled(agent, batch, heads, kv_heads, lens)
    q, kc, vc, table, dlens = (t.float().cpu().numpy() for t in tensors)
    want_q, want_k, want_v, *_ = spec(batch, heads, kv_heads, lens)
    max_pages, poison = max_pages_of(lens), batch * max_pages_of(lens)
    assert np.array_equal(q, want_q) and list(dlens) == list(lens)
    assert np.isnan(kc[poison]).all() and np.isnan(vc[poison]).all()
    used = [int(p) for b in range(batch) for p in table[b, :-(-lens[b] // PAGE)]]
    assert len(set(used)) == len(used) and poison not in used
    for b, length in enumerate(lens):
        assert (table[b, -(-length // PAGE):] == poison).all()
        for cache, want in ((kc, want_k), (vc, want_v)):
            # the sequence's keys through its table; every slot beyond the length is NaN
            got = cache[table[b, :-(-length // PAGE)].astype(int)].transpose(1, 0, 2, 3)
            got = got.reshape(kv_heads, -1, D)
            assert np.array_equal(got[:, :length], want[b, :, :length])
            assert np.isnan(got[:, length:]).all()
    recs, o = _run(agent, *tensors, splits, math.log(2), reps)  # scale_log2 = 1
    want = checksums(batch, heads, kv_heads, lens, splits, reps)
    rc, res = agent.decode_verify(recs, batch, heads, kv_heads, max_pages, lens, splits, reps, SEED)
    assert (rc, res.sweep.bad_waves, res.sweep.waves) == (nodeagent.NA_OK, 0, len(want))
    assert [r.checksum for r in recs] == want
    # O and l are exact, so only the final division rounds: 1 ulp of f32; and
    # nothing of the NaN slots or the poison page got through
    exact = decode(batch, heads, kv_heads, lens, splits)[1]
    err = np.abs(o - exact) / np.spacing(np.abs(exact).astype(np.float32))
    print("largest error in ulp:", err.max())
    assert err.max() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize(ARGS, SHAPES)
def test_gpu_operation_against_float64(agent, batch, heads, kv_heads, lens, splits):
    """The attention sweep's distributions (q and k of deviation 2, v uniform in
    [-1, 1], scale 128^-1/2) and its bound 2^-7 max|v|, whose derivation (P
    rounded to bf16, the rest f32) holds unchanged: the merges are f32. The
    block table is shuffled; the slots beyond a length and the page the unused
    entries name are NaN."""
    gen = torch.Generator().manual_seed(20261126)
    max_pages, n_k = max_pages_of(lens), PAGE * max_pages_of(lens)
    q = (2 * torch.randn((batch, heads, D), generator=gen)).bfloat16()
    k = (2 * torch.randn((batch, kv_heads, n_k, D), generator=gen)).bfloat16()
    v = (2 * torch.rand((batch, kv_heads, n_k, D), generator=gen) - 1).bfloat16()
    places = torch.randperm(batch * max_pages + 1, generator=gen)
    table = places[:-1].reshape(batch, max_pages).to(torch.int32)
    kc = torch.full((batch * max_pages + 1, kv_heads, PAGE, D), float("nan")).bfloat16()
    vc = kc.clone()
    for b, length in enumerate(lens):
        for cache, src in ((kc, k), (vc, v)):
            paged = src[b].clone()
            paged[:, length:] = float("nan")
            cache[table[b].long()] = paged.reshape(kv_heads, max_pages, PAGE, D).transpose(0, 1)
        table[b, -(-length // PAGE):] = places[-1]
    dlens = torch.tensor(lens, dtype=torch.int32)
    _recs, o = _run(agent, q.cuda(), kc.cuda(), vc.cuda(), table.cuda(), dlens.cuda(), splits,
                    D ** -0.5)
    group, err = heads // kv_heads, 0.0
    for b, length in enumerate(lens):
        kb = k[b, :, :length].double().repeat_interleave(group, 0)
        s = torch.einsum("hc,hjc->hj", q[b].double(), kb) / D ** 0.5
        want = torch.einsum("hj,hjc->hc", torch.softmax(s, dim=1),
                            v[b, :, :length].double().repeat_interleave(group, 0))
        err = max(err, np.abs(o[b] - want.numpy()).max())
    atol = 2.0 ** -7 * v.abs().max().item()
    print("largest error", err, "atol", atol)
    assert err <= atol


@pytest.mark.gpu
def test_gpu_a_flipped_key_element_is_pinned_on_the_wave_that_owns_the_tile(agent):
    batch, heads, kv_heads, lens, splits = SHAPES[3]
    q, kc, vc, table, dlens = _filled(agent, batch, heads, kv_heads, lens)
    # key 300 of sequence 0 is in tile 9 of 17: split 1 takes tiles 8..16, its
    # wave 1 tiles 9 and 13; KV head 1 is item 1: record 4 * (1 * 2 + 1) + 1
    b, hk, j = 0, 1, 300
    assert part_of(j, lens[b], splits) == (1, 1)
    column = int(np.flatnonzero(spec(batch, heads, kv_heads, lens)[1][b, hk, j])[0])
    page = int(table[b, j // PAGE])
    kc[page, hk, j % PAGE, column] = -kc[page, hk, j % PAGE, column]
    recs, _o = _run(agent, q, kc, vc, table, dlens, splits, math.log(2))
    want = checksums(batch, heads, kv_heads, lens, splits, 1)
    final = 4 * batch * kv_heads * splits + 1
    assert [i for i, r in enumerate(recs) if r.checksum != want[i]] == [13, final]
    rc, res = agent.decode_verify(recs, batch, heads, kv_heads, max_pages_of(lens), lens, splits,
                                  1, SEED)
    assert (rc, res.sweep.bad_waves, res.sweep.first_bad_wave) == (nodeagent.NA_ERR_VERIFY, 2, 13)
    named = "sequence 0 KV head 1 split 1 wave 1"
    assert named in agent._err() and named in res.describe()


@pytest.mark.gpu
def test_gpu_sweep_and_health_check(agent):
    torch.cuda.synchronize()
    res = agent.decode_sweep(0, batch=4, heads=8, kv_heads=2, max_pages=8, splits=2, reps=2)
    assert res.ok and res.sweep.bad_waves == 0 and res.sweep.waves == 4 * 2 * (4 * 2 + 1)
    assert res.sweep.units_seen >= 1 and res.gbps > 0
    g = agent.check(bw_bytes=1 << 28, decode_sweep=True).gpus[0]
    print("decode sweep:", g.decode_sweep_gbps, "GB/s of KV at", g.decode_sweep_clock_mhz,
          "MHz on", g.decode_sweep_units_seen, "CUs; HBM probe", g.hbm_bw_gbs, "GB/s")
    assert g.decode_sweep_bad_waves == 0 and g.decode_sweep_units_seen >= 1, g.problems
    assert g.decode_sweep_gbps > 0 and g.decode_sweep_clock_mhz > 0
    assert not [p for p in g.problems if "decode" in p]
