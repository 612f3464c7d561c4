"""Chip-wide LDS sweep of the node agent (nodeagent/ldssweep.h).

The reference for every checksum is the numpy simulation below, written from
the specification in the header: it builds the LDS image of each phase word
by word (byte by byte for the LDS-DMA phases, element by element for the
transposed read), walks the 256 threads through their lane-to-address maps
and folds what each would read as the plain recurrence. It shares nothing
with the host code's per-chunk sums, and known answers pin both.

CPU: exported symbols, the host reference against numpy, the verify and its
attribution of bad workgroups to CUs and phases, argument errors, and
check()/report/CLI/chart/docs behaviour against a Python stand-in for the
native library.
GPU (@pytest.mark.gpu, device 0): record checksums at the smallest shapes
that can go wrong, seed dependence, record sanity, localisation on the GPU's
own records (only HOST data is corrupted; nothing on the GPU is provoked),
the default sweep once, and the end-to-end paths.
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
from tests.test_nodeagent_mfmasweep import FakeLib as MfmaFakeLib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEED = nodeagent.DEFAULT_LDS_SWEEP_SEED
PHASES = nodeagent.LDS_SWEEP_PHASES
WHOLE = 160 * 1024
U64 = np.uint64


def _ensure_lib():
    import __graft_entry__ as g

    if not os.path.exists(g.LIB_PATH):
        g.build()
    return g.LIB_PATH


# ---------------------------------------------------------------------------
# numpy simulation of the specification
# ---------------------------------------------------------------------------


def _mix64(x):
    x = x.copy()
    x ^= x >> U64(30)
    x *= U64(0xBF58476D1CE4E5B9)
    x ^= x >> U64(27)
    x *= U64(0x94D049BB133111EB)
    x ^= x >> U64(31)
    return x


@functools.lru_cache(maxsize=None)
def ref_pattern(seed, pat, words):
    """pat(p, j) for j < words, as uint32."""
    with np.errstate(over="ignore"):
        j = np.arange(words, dtype=U64)
        out = (_mix64(U64((seed * G) & M64) + U64(pat << 32) + j) >> U64(32)).astype(np.uint32)
    out.setflags(write=False)
    return out


def _image(seed, pat, W, rot):
    """The LDS words under rotation `rot`: word i = pat(p, (i + 256 rot) mod W)."""
    return np.roll(ref_pattern(seed, pat, W), -256 * rot)


T = np.arange(256)
PERM = (T + 67) & 255


def _fold(c, v):
    with np.errstate(over="ignore"):
        return c * U64(G) + v.astype(U64)


def _total(c):
    return int(c.sum(dtype=U64))


def _read32(lds, chunks, c=None):
    c = np.zeros(256, dtype=U64) if c is None else c
    for k in range(chunks):
        c = _fold(c, lds[256 * k + PERM])
    return c


def _read128(lds, c=None):
    c = np.zeros(256, dtype=U64) if c is None else c
    vec = lds.reshape(-1, 4).astype(U64)
    for k in range(len(vec) // 256):
        got = vec[256 * k + PERM]
        c = _fold(c, got[:, 0] | (got[:, 1] << U64(32)))
        c = _fold(c, got[:, 2] | (got[:, 3] << U64(32)))
    return c


def _dma(seed, lds_bytes, size, rot, before=None, stride=None):
    """LDS words after the LDS-DMA sub-phase of `size` bytes per lane on top
    of the image `before`: wave v of step k writes to its base + stride * l
    the `size` bytes lane l sources from its own address in the buffer. The
    hardware's stride is the size, but 16 at size 12 (measured)."""
    stride = stride or (16 if size == 12 else size)
    source = ref_pattern(seed, 2, lds_bytes // 4).view(np.uint8)
    source = np.concatenate([source, source[:16]])  # only a stride of 12 reads past the end
    lds = np.zeros(lds_bytes, dtype=np.uint8) if before is None else before.view(np.uint8).copy()
    piece = np.arange(size)
    for k in range(lds_bytes // (256 * stride)):
        start = (k * 256 * stride + T * stride + 1024 * rot) % lds_bytes  # per lane
        dest = k * 256 * stride + (T >> 6) * 64 * stride + (T & 63) * stride
        lds[dest[:, None] + piece] = source[start[:, None] + piece]
    return lds.view(np.uint32)


def ref_checksums(seed, workgroup, lds_bytes, iters):
    """The eight phase checksums of one workgroup, in the order of PHASES."""
    W = lds_bytes // 4
    C = W // 256
    rot = workgroup % C
    out = []
    # b32, b128: pattern, then its complement, one checksum through both
    c = None
    for pol in (0, 0xFFFFFFFF):
        c = _read32(_image(seed, 0, W, rot) ^ np.uint32(pol), C, c)
    out.append(_total(c))
    c = None
    for pol in (0, 0xFFFFFFFF):
        c = _read128(_image(seed, 1, W, rot) ^ np.uint32(pol), c)
    out.append(_total(c))
    # dma at 16, 4 and 12 bytes per lane
    out.append(_total(_read128(_dma(seed, lds_bytes, 16, rot))))
    after4 = _dma(seed, lds_bytes, 4, (rot + 1) % C)
    out.append(_total(_read128(after4)))
    out.append(_total(_read128(_dma(seed, lds_bytes, 12, (rot + 2) % C, before=after4))))
    # tr16: lane i of 16-lane group g of wave v receives column i of tile
    # 16k + 4v + g, row q in its element q
    elem = _image(seed, 3, W, rot).view(np.uint16).astype(U64)
    lane = T & 63
    c = np.zeros(256, dtype=U64)
    for k in range(C // 2):
        tile = 16 * k + 4 * (T >> 6) + (lane >> 4)
        value = np.zeros(256, dtype=U64)
        for q in range(4):
            value |= elem[64 * tile + 16 * q + (lane & 15)] << U64(16 * q)
        c = _fold(c, value)
    out.append(_total(c))
    # atomic: every word receives a from its own thread and a >> 16 from a
    # thread of another wave
    lds = np.zeros(W, dtype=np.uint32)
    a = _image(seed, 4, W, rot)
    for k in range(C):
        np.add.at(lds, 256 * k + T, a[256 * k + T])
    for k in range(C):
        i = 256 * k + ((T + 64) & 255)
        np.add.at(lds, i, a[i] >> np.uint32(16))
    out.append(_total(_read32(lds, C)))
    # stream: plain 64-bit sums of every lo and hi, pass after pass
    vec = _image(seed, 5, W, rot).reshape(-1, 4).astype(U64)
    s = np.zeros(256, dtype=U64)
    with np.errstate(over="ignore"):
        for _ in range(iters):
            for k in range(C // 4):
                got = vec[256 * k + T]
                s = s + (got[:, 0] | (got[:, 1] << U64(32))) + (got[:, 2] | (got[:, 3] << U64(32)))
    out.append(_total(s))
    return out


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------

SYMBOLS = ("na_lds_sweep_expected", "na_lds_sweep_run", "na_lds_sweep_verify", "na_lds_sweep")


def test_library_exports_lds_sweep_symbols():
    lib = ctypes.CDLL(_ensure_lib())
    for sym in SYMBOLS + ("na_lds_sweep_allocation",):
        assert hasattr(lib, sym), f"missing symbol {sym}"


def test_seed_constant_spells_its_name():
    assert SEED.to_bytes(8, "big") == b"MI355XLS"
    assert PHASES == ("b32", "b128", "dma16", "dma4", "dma12", "tr16", "atomic", "stream")
    assert ctypes.sizeof(nodeagent.LdsRecord) == 128


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


KNOWN = [
    (0, 0, 4096, 1,
     ["0x97fb1b9594328450", "0xb9d21c0d34850030", "0x3edd027916833ad6", "0x3edd027916833ad6",
      "0x3edd027916833ad6", "0x0e11ebcbc06c2241", "0x45d7b0a8ea177f1f", "0x3cf489454a166526"]),
    (7, 1, 12288, 2,
     ["0x5b2a1b644e3f8730", "0x04292dbf3218d8c8", "0x4c1c4d75d33b43b2", "0x23053e91e05c79c2",
      "0xe858397bce8ba64a", "0x3fd4d71689f1f56f", "0xeab15c20e724852e", "0x24ac98d6ec4fad5a"]),
    (SEED, 5, WHOLE, 5,
     ["0x81c21963f0cae280", "0xecce029947399800", "0x104586b6eede2bca", "0xa85f7480a8642f7a",
      "0x48e0dbea0cd53ec2", "0x54969546991480bf", "0x2c0dc73ee9ffb204", "0x3a78e51b34f875bf"]),
]


@pytest.mark.parametrize("seed,workgroup,lds_bytes,iters,want", KNOWN)
def test_reference_known_answers(cpu_agent, seed, workgroup, lds_bytes, iters, want):
    got = ref_checksums(seed, workgroup, lds_bytes, iters)
    assert [f"{x:#018x}" for x in got] == want
    assert cpu_agent.lds_sweep_expected(workgroup, lds_bytes, iters, seed) == got


@pytest.mark.parametrize("seed", [0, 7, SEED])
@pytest.mark.parametrize("lds_bytes", [4096, 12288, WHOLE])
def test_expected_checksums_match_reference(cpu_agent, seed, lds_bytes):
    for workgroup in (0, 1, 5, 4095):
        for iters in (1, 2, 5):
            want = ref_checksums(seed, workgroup, lds_bytes, iters)
            got = cpu_agent.lds_sweep_expected(workgroup, lds_bytes, iters, seed)
            assert got == want, (workgroup, iters, [PHASES[p] for p in range(8) if got[p] != want[p]])


def test_reference_depends_on_seed_workgroup_and_iters():
    a = ref_checksums(SEED, 1, 12288, 2)
    assert all(x != y for x, y in zip(a, ref_checksums(SEED + 1, 1, 12288, 2)))
    b = ref_checksums(SEED, 2, 12288, 2)
    # one b128-shaped step covers 4 chunks; three of them see the rotation.
    # The stream phase sums and so does not.
    assert [x != y for x, y in zip(a, b)] == [True] * 7 + [False]
    c = ref_checksums(SEED, 1, 12288, 3)
    assert a[:7] == c[:7] and a[7] != c[7]
    # workgroups a whole rotation apart hold the same data
    assert ref_checksums(SEED, 1 + 12, 12288, 2) == a


@pytest.mark.parametrize("lds_bytes", [4096, 12288, WHOLE])
def test_dma12_renews_twelve_of_every_sixteen_bytes(cpu_agent, lds_bytes):
    """The 12-byte width lands at a stride of 16 bytes per lane (measured on
    MI355X), so it covers three words of every vector of the whole region,
    3072 of every 4096 bytes, and the fourth keeps what dma4 left."""
    W, C = lds_bytes // 4, lds_bytes // 1024
    after4 = _dma(SEED, lds_bytes, 4, (3 + 1) % C)
    after12 = _dma(SEED, lds_bytes, 12, (3 + 2) % C, before=after4)
    assert np.array_equal(after4, _image(SEED, 2, W, (3 + 1) % C))
    new = np.arange(W) % 4 < 3
    assert new.sum() * 4 == lds_bytes // 4096 * 3072
    assert np.array_equal(after12[new], _image(SEED, 2, W, (3 + 2) % C)[new])
    assert np.array_equal(after12[~new], after4[~new])
    got = cpu_agent.lds_sweep_expected(3, lds_bytes, 1)[4]
    assert got == ref_checksums(SEED, 3, lds_bytes, 1)[4]
    # packed at 12 bytes per lane it would be another checksum
    packed = _dma(SEED, lds_bytes, 12, (3 + 2) % C, before=after4, stride=12)
    assert got != _total(_read128(packed))


def test_expected_argument_errors(cpu_agent):
    out = (ctypes.c_uint64 * 8)()
    lib = cpu_agent.lib
    u64, i64 = ctypes.c_ulonglong, ctypes.c_longlong
    for lds_bytes, iters, ptr, n in [(0, 1, out, 8), (4095, 1, out, 8), (2048, 1, out, 8),
                                     (WHOLE + 4096, 1, out, 8), (-4096, 1, out, 8),
                                     (4096, 0, out, 8), (4096, 1, None, 8), (4096, 1, out, 7)]:
        rc = lib.na_lds_sweep_expected(u64(1), u64(0), i64(lds_bytes), iters, ptr, n)
        assert rc == nodeagent.NA_ERR_ARG, (lds_bytes, iters, n)
        assert "na_lds_sweep_expected" in cpu_agent._err()


def _unit_of(wg):
    """A made-up placement: workgroups 2j and 2j+1 on one CU."""
    u = wg // 2
    return (u % 8, (u // 8) % 4, (u // 32) % 2, (u // 64) % 16)


LDS, ITERS = 12288, 2


def _records(n, lds_bytes=LDS, iters=ITERS, seed=SEED):
    recs = (nodeagent.LdsRecord * n)()
    for i in range(n):
        r = recs[i]
        r.checksum[:] = ref_checksums(seed, i, lds_bytes, iters)
        r.bad_words, r.first_bad_offset, r.xor_mask = 0, nodeagent.NO_BAD_OFFSET, 0
        r.bad_phase = 0xFFFFFFFF
        # 120, 121, ... bytes per clock
        r.cycles, r.realtime, r.workgroup = iters * lds_bytes // (120 + i), 10, i
        r.xcc, r.se, r.sh, r.cu = _unit_of(i)
    return recs


def test_verify_clean_records(cpu_agent):
    recs = _records(12)
    rc, res = cpu_agent.lds_sweep_verify(recs, LDS, ITERS)
    assert rc == nodeagent.NA_OK and res.ok
    assert (res.workgroups, res.bad_workgroups, res.units_seen, res.bad_units) == (12, 0, 6, 0)
    assert res.first_bad_workgroup == nodeagent.NO_BAD_WORKGROUP and res.bad_cus == []
    assert res.first_bad_phase == "" and res.first_bad_offset == nodeagent.NO_BAD_OFFSET
    # the same records do not verify under other passes, another seed or size
    assert cpu_agent.lds_sweep_verify(recs, LDS, 3)[1].first_bad_phase == "stream"
    assert cpu_agent.lds_sweep_verify(recs, LDS, ITERS, SEED + 1)[1].bad_workgroups == 12
    assert cpu_agent.lds_sweep_verify(recs, 4096, ITERS)[0] == nodeagent.NA_ERR_VERIFY


def test_verify_rate_statistics(cpu_agent):
    recs = _records(12)
    rates = sorted(ITERS * LDS / recs[i].cycles for i in range(12))
    _, res = cpu_agent.lds_sweep_verify(recs, LDS, ITERS)
    assert res.median_bytes_per_clk == pytest.approx(rates[6], rel=1e-12)
    assert res.min_bytes_per_clk == pytest.approx(rates[0], rel=1e-12)
    assert res.max_bytes_per_clk == pytest.approx(rates[-1], rel=1e-12)
    assert 119.9 < rates[0] < 121 and 130 < rates[-1] < 133
    mhz = sorted(recs[i].cycles / 10 * 100.0 for i in range(12))
    assert res.clock_mhz == pytest.approx(mhz[6], rel=1e-12)


@pytest.mark.parametrize("phase", range(8))
def test_verify_one_flipped_bit_names_the_phase(cpu_agent, phase):
    recs = _records(12)
    wg = 3 + phase
    recs[wg].checksum[phase] ^= 1 << (phase * 9)
    rc, res = cpu_agent.lds_sweep_verify(recs, LDS, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY and not res.ok
    assert (res.bad_workgroups, res.bad_units, res.first_bad_workgroup) == (1, 1, wg)
    assert res.first_bad_phase == PHASES[phase] and res.bad_cus == [_unit_of(wg)]
    assert res.first_bad_offset == nodeagent.NO_BAD_OFFSET
    err = cpu_agent._err()
    assert f"1 of 12 workgroups wrong on 1 CU(s), first workgroup {wg} in phase {PHASES[phase]} " \
        f"on {nodeagent.mfma_unit_name(_unit_of(wg))}" in err
    assert PHASES[phase] in res.describe() and nodeagent.mfma_unit_name(_unit_of(wg)) in \
        res.describe()


def test_verify_record_in_the_wrong_place_is_bad(cpu_agent):
    # 0 and 12 share a rotation, hence every checksum: only the index differs
    recs = _records(13)
    recs[12].workgroup = 0
    rc, res = cpu_agent.lds_sweep_verify(recs, LDS, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_workgroups, res.first_bad_workgroup, res.first_bad_phase) == (1, 12, "index")
    assert "phase index" in cpu_agent._err()


def test_verify_in_kernel_bad_count_with_correct_checksums_is_bad(cpu_agent):
    recs = _records(12)
    r = recs[7]
    r.bad_words, r.first_bad_offset, r.xor_mask, r.bad_phase = 2, 0x2A4, 0x00010000, 3
    rc, res = cpu_agent.lds_sweep_verify(recs, LDS, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_workgroups, res.first_bad_workgroup, res.first_bad_phase) == (1, 7, "dma4")
    assert (res.bad_words, res.first_bad_offset, res.xor_mask) == (2, 0x2A4, 0x00010000)
    err = cpu_agent._err()
    # bank = (0x2A4 / 4) mod 64 = 41
    assert "in phase dma4 on " + nodeagent.mfma_unit_name(_unit_of(7)) in err
    assert "first at LDS offset 0x2a4 (bank 41), failing bits 0x00010000" in err
    assert "LDS offset 0x2a4 (bank 41), failing bits 0x00010000" in res.describe()
    # the triple belongs to its own phase: an earlier failing phase reports none
    recs[7].checksum[0] ^= 1
    _, res = cpu_agent.lds_sweep_verify(recs, LDS, ITERS)
    assert res.first_bad_phase == "b32" and res.first_bad_offset == nodeagent.NO_BAD_OFFSET


def test_verify_two_workgroups_of_one_cu_are_one_unit(cpu_agent):
    recs = _records(12)
    recs[4].checksum[1] ^= 2
    recs[5].checksum[6] ^= 1 << 40
    rc, res = cpu_agent.lds_sweep_verify(recs, LDS, ITERS)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_workgroups, res.bad_units, res.first_bad_workgroup) == (2, 1, 4)
    assert res.bad_cus == [_unit_of(4)] and res.first_bad_phase == "b128"
    recs[10].checksum[0] ^= 1
    _, res = cpu_agent.lds_sweep_verify(recs, LDS, ITERS)
    assert (res.bad_workgroups, res.bad_units) == (3, 2)


def test_verify_lists_a_bounded_number_of_cus(cpu_agent):
    n = 2 * (nodeagent.LDS_SWEEP_MAX_LISTED + 2)
    recs = _records(n, 4096, 1)
    for i in range(n):
        recs[i].checksum[5] ^= 1
    _, res = cpu_agent.lds_sweep_verify(recs, 4096, 1)
    assert (res.bad_workgroups, res.bad_units) == (n, n // 2)
    assert res.bad_cus == [_unit_of(2 * i) for i in range(nodeagent.LDS_SWEEP_MAX_LISTED)]
    assert ", ...;" in res.describe()


def test_verify_unwritten_records_are_bad(cpu_agent):
    recs = (nodeagent.LdsRecord * 4)()
    ctypes.memset(recs, 0xFF, ctypes.sizeof(recs))
    rc, res = cpu_agent.lds_sweep_verify(recs, 4096, 1)
    assert rc == nodeagent.NA_ERR_VERIFY and res.bad_workgroups == 4


def test_argument_errors_before_any_hip_call(cpu_agent):
    lib = cpu_agent.lib
    recs = (nodeagent.LdsRecord * 4)()
    ms, gbs = ctypes.c_double(0), ctypes.c_double(0)
    seed, i64 = ctypes.c_ulonglong(SEED), ctypes.c_longlong
    res = nodeagent._LdsSweepResultC()

    def run(workgroups, lds_bytes, iters, out, n_out):
        return lib.na_lds_sweep_run(0, workgroups, i64(lds_bytes), iters, seed, out, i64(n_out),
                                    ctypes.byref(ms))

    for args in [(0, 4096, 1, recs, 4), (-2, 4096, 1, recs, 4), ((1 << 20) + 1, 4096, 1, recs, 4),
                 (2, 4095, 1, recs, 4), (2, 2048, 1, recs, 4), (2, -4096, 1, recs, 4),
                 (2, WHOLE + 4096, 1, recs, 4), (2, 4096, 0, recs, 4), (2, 4096, -1, recs, 4),
                 (2, 4096, (1 << 22) + 1, recs, 4), (2, 4096, 1, None, 4), (2, 4096, 1, recs, 1),
                 (5, 0, 1, recs, 4)]:
        assert run(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_lds_sweep_run" in cpu_agent._err()

    def verify(r, n, lds_bytes, iters, out):
        return lib.na_lds_sweep_verify(r, i64(n), i64(lds_bytes), iters, seed, out)

    for args in [(None, 4, 4096, 1, ctypes.byref(res)), (recs, 0, 4096, 1, ctypes.byref(res)),
                 (recs, 4, 0, 1, ctypes.byref(res)), (recs, 4, 6144, 1, ctypes.byref(res)),
                 (recs, 4, 4096, 0, ctypes.byref(res)), (recs, 4, 4096, 1, None)]:
        assert verify(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_lds_sweep_verify" in cpu_agent._err()

    def sweep(workgroups, lds_bytes, iters, out):
        return lib.na_lds_sweep(0, workgroups, i64(lds_bytes), iters, seed, out, ctypes.byref(gbs))

    for args in [(-1, 0, 0, ctypes.byref(res)), ((1 << 20) + 1, 0, 0, ctypes.byref(res)),
                 (0, 100, 0, ctypes.byref(res)), (0, 0, -1, ctypes.byref(res)),
                 (0, 0, (1 << 22) + 1, ctypes.byref(res)), (0, 0, 0, None)]:
        assert sweep(*args) == nodeagent.NA_ERR_ARG, args
        assert "na_lds_sweep:" in cpu_agent._err()
    with pytest.raises(nodeagent.NodeAgentError):
        cpu_agent.lds_sweep_run(0, workgroups=0)


# -- check() against a Python stand-in library --------------------------------

SICK_CU = (5, 2, 1, 9)


class FakeLib(MfmaFakeLib):
    """The matrix-core sweep's stand-in plus na_lds_sweep. ``lds``: {dev:
    "sick" | "slow" | "fewer"}; default clean. A sick GPU has one CU whose
    four workgroups all fail in the dma12 phase."""

    def __init__(self, ngpu=1, lds=None):
        super().__init__(ngpu=ngpu)
        self.lds_calls = []
        lds = lds or {}

        def na_lds_sweep(dev, workgroups, lds_bytes, iters, seed, res, gbs):
            self.lds_calls.append((dev, workgroups, lds_bytes.value, iters, seed.value))
            kind = lds.get(dev, "ok")
            r = res._obj
            r.workgroups, r.units_seen, r.clock_mhz = 1024, 255 if kind == "fewer" else 256, 2391.7
            r.bad_workgroups, r.bad_units, r.listed = 0, 0, 0
            r.first_bad_workgroup = nodeagent.NO_BAD_WORKGROUP
            r.first_bad_offset, r.first_bad_phase = nodeagent.NO_BAD_OFFSET, 0xFFFFFFFF
            r.median_bytes_per_clk, r.min_bytes_per_clk, r.max_bytes_per_clk = 201.3, 198.266, 203.0
            gbs._obj.value = 12.34 if kind == "slow" else 123251.16
            if kind != "sick":
                return 0
            r.bad_workgroups, r.bad_units, r.first_bad_workgroup, r.listed = 4, 1, 77, 1
            r.first_bad_phase = 4
            r.bad_words, r.first_bad_offset, r.xor_mask = 53, 0x1F8, 0x00000400
            r.bad_list[0][:] = SICK_CU
            r.first_bad_unit[:] = SICK_CU
            return nodeagent.NA_ERR_VERIFY

        self.na_lds_sweep = na_lds_sweep


def _agent(monkeypatch, **kw):
    fake = FakeLib(**kw)
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fake)
    return nodeagent.NodeAgent(), fake


def _sweep_fields(g):
    return (g.lds_sweep_gbs, g.lds_sweep_min_cu_bytes_per_clk, g.lds_sweep_units_seen,
            g.lds_sweep_bad_workgroups)


def test_check_default_never_runs_sweep(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check()
    assert fake.lds_calls == [] and fake.sweep_calls == []
    assert report.healthy, report.problems
    assert _sweep_fields(report.gpus[0]) == (0.0, 0.0, 0, 0)
    assert _sweep_fields(nodeagent.GPUReport(index=0)) == (0.0, 0.0, 0, 0)
    # the stand-in of the matrix-core sweep's tests has no LDS sweep at all
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: MfmaFakeLib())
    assert nodeagent.NodeAgent().check(mfma_sweep=True).healthy


def test_check_clean_sweep_populates_fields(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_LDS_SWEEP_GBS", 80000.0)
    agent, fake = _agent(monkeypatch)
    report = agent.check(lds_sweep=True)
    assert fake.lds_calls == [(0, 0, 0, 0, SEED)] and fake.sweep_calls == []
    g = report.gpus[0]
    assert report.healthy and g.healthy, report.problems
    assert _sweep_fields(g) == (123251.2, 198.27, 256, 0)
    assert nodeagent.node_condition_from_report(report)["status"] == "True"


def test_check_units_seen_below_cus_is_reported_not_a_problem(monkeypatch):
    agent, _ = _agent(monkeypatch, lds={0: "fewer"})
    report = agent.check(lds_sweep=True)
    assert report.gpus[0].lds_sweep_units_seen == 255 < report.gpus[0].cus
    assert report.healthy, report.problems


def test_check_eight_gpus_one_sick_cu(monkeypatch):
    agent, fake = _agent(monkeypatch, ngpu=8, lds={3: "sick"})
    report = agent.check(expect_gpus=8, lds_sweep=True)
    assert [c[0] for c in fake.lds_calls] == list(range(8))
    assert report.problems == [
        "gpu3: LDS sweep: 4 of 1024 workgroups wrong on 1 CU(s): xcc5.se2.sh1.cu9; first in "
        "phase dma12, 53 bad words, first at LDS offset 0x1f8 (bank 62), failing bits 0x00000400"
    ]
    assert not report.healthy
    assert [g.healthy for g in report.gpus] == [i != 3 for i in range(8)]
    assert [g.lds_sweep_bad_workgroups for g in report.gpus] == [4 * (i == 3) for i in range(8)]
    assert nodeagent.node_condition_from_report(report)["status"] == "False"


def test_check_low_rate_flags_a_problem(monkeypatch):
    monkeypatch.setattr(nodeagent, "MIN_LDS_SWEEP_GBS", 80000.0)
    agent, _ = _agent(monkeypatch, lds={0: "slow"})
    report = agent.check(lds_sweep=True)
    assert report.gpus[0].problems == ["LDS sweep 12.3 GB/s below floor 80000.0"]
    assert not report.healthy
    agent, _ = _agent(monkeypatch)
    assert agent.check(lds_sweep=True).healthy


def test_floor_is_derived_from_the_profile():
    """0.70 x the median of the profile's per-process figures."""
    with open(os.path.join(ROOT, "profiles", "lds_sweep_mi355x.txt")) as f:
        runs = [float(x) for line in f if line.startswith("gbs ") for x in line.split()[1:]]
    assert len(runs) >= 5
    assert nodeagent.MIN_LDS_SWEEP_GBS == pytest.approx(0.70 * float(np.median(runs)), abs=0.06)


def test_cli_flag_reaches_check(monkeypatch, capsys):
    _, fake = _agent(monkeypatch)
    assert nodeagent.main(["--lds-sweep"]) == 0
    assert [c[0] for c in fake.lds_calls] == [0]
    assert json.loads(capsys.readouterr().out)["gpus"][0]["lds_sweep_units_seen"] == 256
    _, fake = _agent(monkeypatch)
    assert nodeagent.main([]) == 0
    assert fake.lds_calls == []
    capsys.readouterr()


def test_chart_passes_lds_sweep_only_when_true():
    import yaml

    chart = os.path.join(ROOT, "charts", "gpu-provisioner-amd")
    with open(os.path.join(chart, "values.yaml")) as f:
        values = yaml.safe_load(f)
    assert values["nodeAgent"]["ldsSweep"] is False
    with open(os.path.join(chart, "templates", "amd-gpu-node-stack.yaml")) as f:
        text = f.read()
    start = text.index("{{- if .Values.nodeAgent.ldsSweep }}")
    end = text.index("{{- end }}", start)
    assert "--lds-sweep \\" in text[start:end]
    assert text.count("--lds-sweep") == 1  # nowhere outside the guard


def test_docs_cover_every_new_report_field():
    with open(os.path.join(ROOT, "docs", "METRICS.md")) as f:
        metrics = f.read()
    for name in ("lds_sweep_gbs", "lds_sweep_min_cu_bytes_per_clk", "lds_sweep_units_seen",
                 "lds_sweep_bad_workgroups"):
        assert name in metrics, name
        assert hasattr(nodeagent.GPUReport(index=0), name)


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


_runs = {}


def _run(agent, workgroups, lds_bytes, iters, seed=SEED):
    """One launch per distinct shape, shared by the tests; read-only.
    lds_bytes 0 is resolved to the device's allocation."""
    lds_bytes = lds_bytes or agent.lds_sweep_allocation(0)
    key = (workgroups, lds_bytes, iters, seed)
    if key not in _runs:
        torch.cuda.synchronize()
        _runs[key] = agent.lds_sweep_run(0, workgroups, lds_bytes, iters, seed)[0]
    return _runs[key], lds_bytes


_sweeps = []


def _default_sweep(agent):
    if not _sweeps:
        torch.cuda.synchronize()
        _sweeps.append(agent.lds_sweep(0))
    return _sweeps[0]


# 4096: one LDS-DMA wave-instruction per wave at 16 and 12 bytes, one step of
# every 128-bit loop; 12288: several steps, rotations differ between the
# workgroups; whole: every address of the allocation, and the stream loop's
# pipelined path (a multiple of eight steps)
@pytest.mark.gpu
@pytest.mark.parametrize("workgroups,lds_bytes,iters", [(1, 4096, 1), (3, 12288, 2), (3, 0, 1)])
def test_gpu_record_checksums_match_reference(agent, workgroups, lds_bytes, iters):
    recs, lds_bytes = _run(agent, workgroups, lds_bytes, iters)
    assert len(recs) == workgroups
    for wg, r in enumerate(recs):
        want = ref_checksums(SEED, wg, lds_bytes, iters)
        got = list(r.checksum)
        print(f"workgroup {wg} of {lds_bytes} bytes:", [f"{x:#x}" for x in got])
        assert got == want, [PHASES[p] for p in range(8) if got[p] != want[p]]


@pytest.mark.gpu
def test_gpu_seed_changes_every_phase(agent):
    recs, _ = _run(agent, 3, 12288, 2)
    other, _ = _run(agent, 3, 12288, 2, seed=7)
    for wg in range(3):
        assert all(a != b for a, b in zip(recs[wg].checksum, other[wg].checksum))
        assert list(other[wg].checksum) == ref_checksums(7, wg, 12288, 2)


@pytest.mark.gpu
def test_gpu_record_sanity(agent):
    recs, _ = _run(agent, 3, 0, 1)
    assert [r.workgroup for r in recs] == [0, 1, 2]
    for r in recs:
        assert r.xcc < 8 and r.se < 4 and r.sh < 2 and r.cu < 16
        assert r.cycles > 0 and r.realtime > 0
        assert r.bad_words == 0 and r.first_bad_offset == nodeagent.NO_BAD_OFFSET
        assert r.bad_phase == 0xFFFFFFFF and r.xor_mask == 0


@pytest.mark.gpu
def test_gpu_localisation_on_own_records(agent):
    src, lds_bytes = _run(agent, 3, 0, 1)
    rc, res = agent.lds_sweep_verify(src, lds_bytes, 1)
    assert rc == nodeagent.NA_OK and res.ok and res.workgroups == 3
    recs = (nodeagent.LdsRecord * len(src))()
    ctypes.memmove(recs, src, ctypes.sizeof(src))  # the shared run stays as it came back
    recs[1].checksum[5] ^= 1 << 17
    rc, res = agent.lds_sweep_verify(recs, lds_bytes, 1)
    assert rc == nodeagent.NA_ERR_VERIFY
    unit = (recs[1].xcc, recs[1].se, recs[1].sh, recs[1].cu)
    assert (res.bad_workgroups, res.bad_units, res.first_bad_workgroup) == (1, 1, 1)
    assert res.bad_cus == [unit] and res.first_bad_phase == "tr16"
    assert nodeagent.mfma_unit_name(unit) in agent._err() and "phase tr16" in agent._err()


@pytest.mark.gpu
def test_gpu_default_sweep(agent):
    res = _default_sweep(agent)
    _, _, _, cus = agent.device_info(0)
    peak = nodeagent.LDS_SWEEP_PEAK_BYTES_PER_CLK
    ceiling = cus * peak * res.clock_mhz / 1000.0
    print(f"lds_sweep: {res.gbs:.1f} GB/s (ceiling {ceiling:.1f}), per CU median "
          f"{res.median_bytes_per_clk:.2f} min {res.min_bytes_per_clk:.2f} max "
          f"{res.max_bytes_per_clk:.2f} B/clk, {res.clock_mhz:.0f} MHz, {res.units_seen} of "
          f"{cus} CUs, {res.workgroups} workgroups")
    assert res.ok, res.describe()
    assert res.workgroups == 4 * cus and res.bad_workgroups == 0 and res.bad_cus == []
    assert res.units_seen == cus
    assert res.gbs > nodeagent.MIN_LDS_SWEEP_GBS > 0
    # the physical ceiling: a figure above it means the timing is wrong
    assert 0 < res.min_bytes_per_clk <= res.median_bytes_per_clk <= res.max_bytes_per_clk <= peak
    assert res.gbs <= ceiling


@pytest.mark.gpu
def test_gpu_check_with_sweep(agent):
    torch.cuda.synchronize()
    report = agent.check(bw_bytes=1 << 28, lds_sweep=True)
    g0 = report.gpus[0]
    assert g0.healthy, g0.problems
    assert g0.lds_sweep_gbs > nodeagent.MIN_LDS_SWEEP_GBS
    assert 0 < g0.lds_sweep_min_cu_bytes_per_clk <= nodeagent.LDS_SWEEP_PEAK_BYTES_PER_CLK
    assert g0.lds_sweep_units_seen == g0.cus and g0.lds_sweep_bad_workgroups == 0


@pytest.mark.gpu
def test_gpu_cli_lds_sweep():
    _ensure_lib()
    proc = subprocess.run(
        [sys.executable, "-m", "gpu_provisioner_amd.nodeagent", "--json",
         "--bw-bytes", "268435456", "--lds-sweep"],
        capture_output=True,
        text=True,
        cwd=ROOT,
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    report = json.loads(proc.stdout)
    assert report["healthy"] is True
    g0 = report["gpus"][0]
    assert g0["lds_sweep_bad_workgroups"] == 0 and g0["lds_sweep_gbs"] > 0
    assert g0["lds_sweep_units_seen"] == g0["cus"]
