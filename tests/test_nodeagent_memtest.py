"""HBM data-integrity test (pattern fill / verify / verify+invert) of the
node agent.

The reference for every data check is the numpy implementation of the
pattern below — written from the specification, independent of the kernel,
and pinned by known answers.

CPU: exported symbols, the reference itself, and check()/report/condition
behaviour against a Python stand-in for the native library.
GPU (@pytest.mark.gpu, device 0): bit-exact fill, clean verify, single- and
multi-bit injection, verify+invert, a fully corrupt region, argument checks
and the end-to-end paths. Corrupted DATA is injected; nothing here provokes
a GPU fault.
"""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

# torch is imported here, at collection, before any test in the session loads
# the agent library: both link libamdhip64.so.7, and the GPU tests below hand
# torch's device pointers to the library, so the process must hold ONE HIP
# runtime — torch's, the order smoke() uses. With the agent library loaded
# first the process ends up with two runtimes and torch sees no GPU.
try:
    import torch
except ImportError:  # CPU-only environment: the GPU tests cannot run there
    torch = None

from gpu_provisioner_amd import nodeagent
from gpu_provisioner_amd.apis import v1 as karpv1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M64 = (1 << 64) - 1
NO_OFFSET = M64  # first_bad_offset when nothing mismatched


def _ensure_lib():
    import __graft_entry__ as g

    if not os.path.exists(g.LIB_PATH):
        g.build()
    return g.LIB_PATH


# ---------------------------------------------------------------------------
# numpy reference of the pattern
# ---------------------------------------------------------------------------


def _mix64(x):
    x = x.copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def ref_words(v, seed, invert=False):
    """Pattern for vector indices ``v`` (array-like of ints < 2^64) as a
    uint64 array of 2*len(v) little-endian words: lo0, hi0, lo1, hi1, ..."""
    v = np.asarray(v, dtype=np.uint64)
    base = np.uint64((seed * 0x9E3779B97F4A7C15) & M64)
    with np.errstate(over="ignore"):
        h = _mix64(v + base)
    out = np.empty(2 * v.size, dtype=np.uint64)
    out[0::2] = h
    out[1::2] = ~((h << np.uint64(32)) | (h >> np.uint64(32)))
    if invert:
        out = ~out
    return out


@functools.lru_cache(maxsize=None)
def ref_region(nvec, seed, invert=False):
    """Reference for a whole region; computed once, shared, read-only."""
    out = ref_words(np.arange(nvec, dtype=np.uint64), seed, invert)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------


def test_library_exports_memtest_symbols():
    lib = ctypes.CDLL(_ensure_lib())
    for sym in ("na_mem_info", "na_memtest_fill", "na_memtest_verify", "na_hbm_memtest"):
        assert hasattr(lib, sym), f"missing symbol {sym}"


@pytest.mark.parametrize(
    "v,seed,invert,lo,hi",
    [
        (1, 0, False, 0x5692161D100B05E5, 0xEFF4FA1AA96DE9E2),
        (0, 1, False, 0xE220A8397B1DCDAF, 0x84E232501DDF57C6),
        (12345, 7, False, 0x1F6622B40CB38E42, 0xF34C71BDE099DD4B),
        (12345, 7, True, 0xE099DD4BF34C71BD, 0x0CB38E421F6622B4),
        ((1 << 32) + 3, 0xDEADBEEF, False, 0xFDFDFD2A257AE8B4, 0xDA85174B020202D5),
    ],
)
def test_reference_known_answers(v, seed, invert, lo, hi):
    w = ref_words([v], seed, invert)
    assert (int(w[0]), int(w[1])) == (lo, hi), f"got {int(w[0]):#x}, {int(w[1]):#x}"


def test_reference_zero_seed_zero_vector_is_degenerate():
    """Why the agent's default seed is non-zero."""
    w = ref_words([0], 0)
    assert (int(w[0]), int(w[1])) == (0, M64)
    assert nodeagent.DEFAULT_MEMTEST_SEED != 0


def test_reference_lo_distinct_and_nonzero():
    """mix64 is a bijection: no two vectors of a region share `lo`, so an
    aliased address line is a mismatch. Seed 7 has no zero word."""
    w = ref_region(1 << 22, 7)
    assert np.unique(w[0::2]).size == 1 << 22
    assert np.count_nonzero(w) == w.size


class FakeLib:
    """Python stand-in for the native library: every na_* function check()
    calls, filling byref() out-arguments through ``._obj``. Functions are
    plain attributes so ``restype`` can be set on them as on a CDLL's."""

    def __init__(self, ngpu=1, free=200 << 30, memtest=None):
        # memtest: {dev: ("ok"|"bad"|"alloc", ...)}; default clean
        self.memtest_calls = []
        self.error = b""
        memtest = memtest or {}

        def _val(x):
            return getattr(x, "value", x)

        def na_last_error():
            return self.error

        def na_device_count(n):
            n._obj.value = ngpu
            return 0

        def na_device_info(dev, name, name_len, arch, arch_len, hbm, cus, clk):
            name.value = b"AMD Instinct MI355X"
            arch.value = b"gfx950:sramecc+:xnack-"
            hbm._obj.value = 288 << 30
            cus._obj.value = 256
            clk._obj.value = 2400000
            return 0

        def bandwidth(gbs):
            def fn(dev, bytes_, iters, out):
                out._obj.value = gbs
                return 0

            return fn

        def ok(dev):
            return 0

        def na_lds_selftest(dev, tested):
            tested._obj.value = 160 * 1024
            return 0

        def na_p2p_matrix(n, buf):
            for i in range(n * n):
                buf[i] = 1
            return 0

        def na_mem_info(dev, free_b, total_b):
            free_b._obj.value = free
            total_b._obj.value = 288 << 30
            return 0

        def na_hbm_memtest(dev, bytes_, rounds, seed, res, gbs):
            nbytes = _val(bytes_)
            self.memtest_calls.append((dev, nbytes, rounds, _val(seed)))
            kind = memtest.get(dev, ("ok",))
            if kind[0] == "alloc":
                self.error = b"hbm memtest: allocation failed after 0 of 1024 bytes: out of memory"
                return nodeagent.NA_ERR_HIP
            r = res._obj
            r.bytes_tested = nbytes
            gbs._obj.value = 4321.04
            if kind[0] == "bad":
                r.bad_words, r.first_bad_offset, r.xor_mask = kind[1:]
                return nodeagent.NA_ERR_VERIFY
            r.bad_words, r.first_bad_offset, r.xor_mask = 0, NO_OFFSET, 0
            return 0

        self.na_last_error = na_last_error
        self.na_device_count = na_device_count
        self.na_device_info = na_device_info
        self.na_hbm_bandwidth = bandwidth(6000.0)
        self.na_sdma_bandwidth = bandwidth(4900.0)
        for name in (
            "na_fma_selftest", "na_mfma_selftest", "na_mfma_bf16_selftest",
            "na_mfma_fp8_selftest", "na_mfma_bf16_tile_check", "na_mfma_fp8_tile_check",
            "na_mfma_i8_tile_check", "na_mfma_f16_tile_check", "na_mfma_mx_tile_check",
            "na_mfma_bf16_tile32_check",
        ):
            setattr(self, name, ok)
        self.na_lds_selftest = na_lds_selftest
        self.na_p2p_matrix = na_p2p_matrix
        self.na_mem_info = na_mem_info
        self.na_hbm_memtest = na_hbm_memtest


def _agent(monkeypatch, **kw):
    fake = FakeLib(**kw)
    monkeypatch.setattr(nodeagent, "_load_lib", lambda: fake)
    return nodeagent.NodeAgent(), fake


def test_check_default_never_runs_memtest(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check()
    assert fake.memtest_calls == []
    assert report.healthy, report.problems
    g = report.gpus[0]
    assert (g.hbm_memtest_bytes, g.hbm_memtest_bad_words, g.hbm_memtest_gbs,
            g.hbm_memtest_skipped) == (0, 0, 0.0, "")
    # the defaults of a report built by hand are the same "not run"
    d = nodeagent.GPUReport(index=0)
    assert (d.hbm_memtest_bytes, d.hbm_memtest_bad_words, d.hbm_memtest_gbs,
            d.hbm_memtest_skipped) == (0, 0, 0.0, "")


def test_check_clean_memtest_populates_fields(monkeypatch):
    agent, fake = _agent(monkeypatch)
    report = agent.check(memtest_bytes=8 << 30)
    assert fake.memtest_calls == [(0, 8 << 30, 1, nodeagent.DEFAULT_MEMTEST_SEED)]
    g = report.gpus[0]
    assert report.healthy and g.healthy, report.problems
    assert g.hbm_memtest_bytes == 8 << 30
    assert g.hbm_memtest_bad_words == 0
    assert g.hbm_memtest_gbs == 4321.0
    assert g.hbm_memtest_skipped == ""
    assert nodeagent.node_condition_from_report(report)["status"] == "True"


def test_check_bad_words_problem_string_and_condition(monkeypatch):
    agent, _ = _agent(monkeypatch, memtest={0: ("bad", 3, 0x40, 0x8001)})
    report = agent.check(memtest_bytes=1024)
    want = ("HBM memtest: 3 bad 64-bit words in 1024 bytes, first at offset 0x40, "
            "failing bits 0x8001")
    g = report.gpus[0]
    assert g.problems == [want]
    assert not g.healthy and not report.healthy
    assert g.hbm_memtest_bad_words == 3 and g.hbm_memtest_bytes == 1024
    assert report.problems == [f"gpu0: {want}"]
    assert nodeagent.node_condition_from_report(report) == {
        "type": karpv1.AMD_GPU_HEALTHY_CONDITION_TYPE,
        "status": "False",
        "reason": "GPUUnhealthy",
        "message": f"gpu0: {want}",
    }


def test_check_allocation_failure_is_skipped_not_unhealthy(monkeypatch):
    agent, fake = _agent(monkeypatch, memtest={0: ("alloc",)})
    report = agent.check(memtest_bytes=1 << 30)
    g = report.gpus[0]
    assert len(fake.memtest_calls) == 1
    assert "allocation failed" in g.hbm_memtest_skipped
    assert g.hbm_memtest_bytes == 0 and g.hbm_memtest_bad_words == 0
    assert g.healthy and report.healthy, report.problems


def test_check_too_small_clamp_is_skipped_not_unhealthy(monkeypatch):
    agent, fake = _agent(monkeypatch, free=17)  # 90 % of 17 is 15 < one vector
    report = agent.check(memtest_bytes=1 << 30)
    g = report.gpus[0]
    assert fake.memtest_calls == []
    assert g.hbm_memtest_skipped and "17" in g.hbm_memtest_skipped
    assert g.hbm_memtest_bytes == 0
    assert g.healthy and report.healthy, report.problems


def test_check_clamps_to_90_percent_of_free(monkeypatch):
    agent, fake = _agent(monkeypatch, free=1000)
    report = agent.check(memtest_bytes=1 << 30)
    # 90 % of 1000 = 900, rounded down to whole 16-byte vectors
    assert [c[1] for c in fake.memtest_calls] == [896]
    assert report.gpus[0].hbm_memtest_bytes == 896
    # a request under the clamp goes through as asked
    agent, fake = _agent(monkeypatch, free=1000)
    agent.check(memtest_bytes=512)
    assert [c[1] for c in fake.memtest_calls] == [512]


def test_check_eight_gpus_one_fails_memtest(monkeypatch):
    agent, fake = _agent(monkeypatch, ngpu=8, memtest={5: ("bad", 1, 0x1238, 1 << 63)})
    report = agent.check(expect_gpus=8, memtest_bytes=1 << 20)
    assert report.gpu_count == 8 and len(report.gpus) == 8
    assert [c[0] for c in fake.memtest_calls] == list(range(8))
    want = ("gpu5: HBM memtest: 1 bad 64-bit words in 1048576 bytes, first at offset 0x1238, "
            "failing bits 0x8000000000000000")
    assert report.problems == [want]
    assert not report.healthy
    assert [g.healthy for g in report.gpus] == [i != 5 for i in range(8)]
    assert report.xgmi_p2p == [[1] * 8 for _ in range(8)]
    cond = nodeagent.node_condition_from_report(report)
    assert cond["status"] == "False" and cond["message"] == want


def test_chart_passes_memtest_bytes_only_when_set():
    import yaml

    chart = os.path.join(ROOT, "charts", "gpu-provisioner-amd")
    with open(os.path.join(chart, "values.yaml")) as f:
        values = yaml.safe_load(f)
    assert values["nodeAgent"]["memtestBytes"] == 0
    with open(os.path.join(chart, "templates", "amd-gpu-node-stack.yaml")) as f:
        text = f.read()
    start = text.index("{{- if .Values.nodeAgent.memtestBytes }}")
    end = text.index("{{- end }}", start)
    assert "--memtest-bytes {{" in text[start:end]
    assert text.count("--memtest-bytes") == 1  # nowhere outside the guard


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------

GUARD_VECS = 4
SENTINEL = 0x5A5AA5A5C3C33C3C
SEED = 7

# vectors per workgroup tile of the kernels (1024 threads x 4 vectors in
# flight): 4095/4096/4097 sit either side of the full-tile/tail-tile path
TILE = 4096
SIZES = [1, 63, 1024, TILE - 1, TILE, 4 * 1024 + 1, 3 * 4096 + 1027, (1 << 22) + 7]
BIG = (1 << 22) + 7
MIXED = 3 * 4096 + 1027  # three full tiles and a 1027-vector tail


class Region:
    """``nvec`` vectors of device memory between sentinel guards."""

    def __init__(self, nvec):
        self.nvec = nvec
        self.buf = torch.full(
            (2 * (nvec + 2 * GUARD_VECS),), _signed(SENTINEL), dtype=torch.int64, device="cuda:0"
        )
        self.words = self.buf[2 * GUARD_VECS: 2 * (GUARD_VECS + nvec)]
        self.ptr = self.buf.data_ptr() + 16 * GUARD_VECS
        self.bytes = 16 * nvec
        assert self.words.data_ptr() == self.ptr

    def sync(self):
        torch.cuda.synchronize()

    def host(self):
        self.sync()
        return self.words.cpu().numpy().view(np.uint64)

    def guards_intact(self):
        self.sync()
        g = torch.cat([self.buf[: 2 * GUARD_VECS], self.buf[-2 * GUARD_VECS:]])
        return bool((g == _signed(SENTINEL)).all().item())

    def flip(self, word, bit):
        self.words[word] ^= _signed(1 << bit)
        self.sync()


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _filled(agent, nvec, invert=False):
    r = Region(nvec)
    r.sync()
    assert agent.memtest_fill(0, r.ptr, r.bytes, SEED, invert) == nodeagent.NA_OK
    return r


def _verify(agent, r, invert=False, flip=False):
    r.sync()
    return agent.memtest_verify(0, r.ptr, r.bytes, SEED, invert, flip)


@pytest.mark.gpu
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("nvec", SIZES)
def test_gpu_fill_matches_reference(agent, nvec, invert):
    r = _filled(agent, nvec, invert)
    assert np.array_equal(r.host(), ref_region(nvec, SEED, invert))
    assert r.guards_intact()


@pytest.mark.gpu
@pytest.mark.parametrize("nvec", SIZES)
def test_gpu_verify_clean(agent, nvec):
    r = _filled(agent, nvec)
    rc, res = _verify(agent, r)
    assert rc == nodeagent.NA_OK
    assert (res.bytes_tested, res.bad_words, res.first_bad_offset, res.xor_mask) == (
        16 * nvec, 0, NO_OFFSET, 0)
    # and the inverted fill verifies against the inverted pattern only
    r = _filled(agent, nvec, invert=True)
    rc, res = _verify(agent, r, invert=True)
    assert rc == nodeagent.NA_OK and res.bad_words == 0
    rc, res = _verify(agent, r, invert=False)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert res.bad_words == 2 * nvec and res.first_bad_offset == 0 and res.xor_mask == M64


# (word, bit): word 0 bit 0; last word bit 63; an odd (hi) word inside a
# full tile's unrolled body; a word in the tail tile
INJECTIONS = [
    (0, 0),
    (2 * MIXED - 1, 63),
    (2 * 5000 + 1, 17),
    (2 * (3 * 4096 + 500), 40),
]


@pytest.mark.gpu
@pytest.mark.parametrize("word,bit", INJECTIONS)
def test_gpu_single_bit_injection(agent, word, bit):
    r = _filled(agent, MIXED)
    r.flip(word, bit)
    rc, res = _verify(agent, r)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_words, res.first_bad_offset, res.xor_mask) == (1, 8 * word, 1 << bit)
    err = agent._err()
    assert "1 bad 64-bit words" in err and f"offset {8 * word:#x}" in err
    assert f"{1 << bit:016x}" in err


@pytest.mark.gpu
def test_gpu_single_bit_injection_single_vector(agent):
    r = _filled(agent, 1)
    r.flip(1, 63)
    rc, res = _verify(agent, r)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_words, res.first_bad_offset, res.xor_mask) == (1, 8, 1 << 63)


@pytest.mark.gpu
def test_gpu_three_flips(agent):
    r = _filled(agent, MIXED)
    picks = INJECTIONS[1:]
    for word, bit in picks:
        r.flip(word, bit)
    rc, res = _verify(agent, r)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert res.bad_words == 3
    assert res.first_bad_offset == 8 * min(w for w, _ in picks)
    assert res.xor_mask == (1 << 63) | (1 << 17) | (1 << 40)


@pytest.mark.gpu
@pytest.mark.parametrize("nvec", SIZES)
def test_gpu_verify_flip_clean(agent, nvec):
    r = _filled(agent, nvec)
    rc, res = _verify(agent, r, flip=True)
    assert rc == nodeagent.NA_OK
    assert (res.bad_words, res.first_bad_offset, res.xor_mask) == (0, NO_OFFSET, 0)
    assert np.array_equal(r.host(), ref_region(nvec, SEED, True))
    assert r.guards_intact()


@pytest.mark.gpu
@pytest.mark.parametrize("word,bit", INJECTIONS)
def test_gpu_verify_flip_reports_and_repairs(agent, word, bit):
    """The flip pass stores the complement of the EXPECTED value, so a bad
    read is reported once and does not poison the next pass."""
    r = _filled(agent, MIXED)
    r.flip(word, bit)
    rc, res = _verify(agent, r, flip=True)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert (res.bad_words, res.first_bad_offset, res.xor_mask) == (1, 8 * word, 1 << bit)
    assert np.array_equal(r.host(), ref_region(MIXED, SEED, True))
    assert r.guards_intact()
    rc, res = _verify(agent, r, invert=True)
    assert rc == nodeagent.NA_OK and res.bad_words == 0


@pytest.mark.gpu
def test_gpu_fully_corrupt_region_is_bounded(agent):
    """Every word wrong: the per-thread accounting touches the global result
    a bounded number of times, so the call simply returns."""
    r = _filled(agent, BIG)
    r.words.zero_()
    ref = ref_region(BIG, SEED)
    nz = np.flatnonzero(ref)
    rc, res = _verify(agent, r)
    assert rc == nodeagent.NA_ERR_VERIFY
    assert res.bad_words == nz.size
    assert res.first_bad_offset == 8 * int(nz[0])
    assert res.xor_mask == int(np.bitwise_or.reduce(ref))
    assert r.guards_intact()


@pytest.mark.gpu
def test_gpu_argument_checks(agent):
    r = _filled(agent, 63)
    before = r.host().copy()
    bad = [(r.ptr + 8, r.bytes - 16), (r.ptr, 0), (r.ptr, 8), (r.ptr, r.bytes - 8)]
    for ptr, nbytes in bad:
        r.sync()
        assert agent.memtest_fill(0, ptr, nbytes, SEED + 1, False) == nodeagent.NA_ERR_ARG
        r.sync()
        rc, _ = agent.memtest_verify(0, ptr, nbytes, SEED, False, True)
        assert rc == nodeagent.NA_ERR_ARG
    # nothing was launched: memory is as the fill left it
    assert np.array_equal(r.host(), before)
    assert r.guards_intact()


@pytest.mark.gpu
def test_gpu_mem_info(agent):
    free, total = agent.mem_info(0)
    assert 0 < free <= total and total > 200e9


@pytest.mark.gpu
def test_gpu_hbm_memtest_end_to_end(agent):
    torch.cuda.synchronize()
    res = agent.hbm_memtest(0, 1 << 30)
    assert res.ok and res.bad_words == 0
    assert res.first_bad_offset == NO_OFFSET and res.xor_mask == 0
    assert res.bytes_tested == 1 << 30
    assert res.gbs > 0
    print(f"hbm_memtest 1 GiB: {res.gbs:.0f} GB/s aggregate")
    # a region that is no whole number of tiles, over two rounds
    res = agent.hbm_memtest(0, 16 * MIXED + 5, rounds=2)
    assert res.ok and res.bytes_tested == 16 * MIXED


@pytest.mark.gpu
def test_gpu_check_with_memtest(agent):
    torch.cuda.synchronize()
    report = agent.check(bw_bytes=1 << 28, memtest_bytes=1 << 28)
    g0 = report.gpus[0]
    assert g0.healthy, g0.problems
    assert g0.hbm_memtest_bytes == 1 << 28
    assert g0.hbm_memtest_bad_words == 0
    assert g0.hbm_memtest_gbs > 0
    assert g0.hbm_memtest_skipped == ""


@pytest.mark.gpu
def test_gpu_cli_memtest_bytes():
    _ensure_lib()
    proc = subprocess.run(
        [sys.executable, "-m", "gpu_provisioner_amd.nodeagent", "--json",
         "--bw-bytes", "268435456", "--memtest-bytes", "268435456"],
        capture_output=True,
        text=True,
        cwd=ROOT,
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    report = json.loads(proc.stdout)
    assert report["healthy"] is True
    g0 = report["gpus"][0]
    assert g0["hbm_memtest_bytes"] == 268435456
    assert g0["hbm_memtest_bad_words"] == 0
    assert g0["hbm_memtest_skipped"] == ""
