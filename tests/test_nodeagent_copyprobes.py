"""The node agent's three copy probes (na_hbm_bandwidth, na_sdma_bandwidth,
na_p2p_bandwidth) and the pointer-level launch of the HBM probe's kernel
(na_copy_run -> copy_f4_kernel, nodeagent/agent.hip).

What a copy has to do needs no formula: the destination equals the source
bit for bit, and nothing else changes. The source holds the memtest pattern
(nodeagent/memtest.h), whose 64-bit words are distinct across a region, so a
vector that lands in the wrong place is a mismatch; the small cases also hold
the source against the numpy copy of that pattern below, written from its
specification. Source and destination sit between guard vectors of two
DIFFERENT values (a vector copied from one past the source's end to one past
the destination's would otherwise write a guard's value onto a guard), and the
destination starts out as a third.

CPU: every argument error of na_copy_run, of the three probes and of
na_p2p_matrix comes back as NA_ERR_ARG with the function and the bad value in
na_last_error, ahead of any HIP call (without a device a HIP call would
return NA_ERR_HIP instead).
GPU (@pytest.mark.gpu, device 0): na_copy_run at the smallest shapes at which
each path of the kernel's indexing can go wrong, and at the probe's own shape;
the probes end to end, with their destination verified.

The probes' buffers are their own and cannot be corrupted from outside, so
there is no negative end-to-end test of them here: that a wrong word is
detected rests on the MT_VERIFY kernel, which the injection tests of
tests/test_nodeagent_memtest.py cover.
"""
import ctypes
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

M64 = (1 << 64) - 1


def _ensure_lib():
    import __graft_entry__ as g

    if not os.path.exists(g.LIB_PATH):
        g.build()
    return g.LIB_PATH


# ---------------------------------------------------------------------------
# numpy reference of the source pattern (memtest.h: normative there)
# ---------------------------------------------------------------------------


def ref_words(nvec, seed):
    """Vectors 0..nvec-1 of the pattern as 2*nvec uint64 words: lo = mix64(v
    + seed * 0x9E3779B97F4A7C15), hi = ~swap32(lo); mix64 is the splitmix64
    finaliser."""
    with np.errstate(over="ignore"):
        x = np.arange(nvec, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) & M64)
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    out = np.empty(2 * nvec, dtype=np.uint64)
    out[0::2] = x
    out[1::2] = ~((x << np.uint64(32)) | (x >> np.uint64(32)))
    return out


def test_reference_known_answers():
    """The vectors tests/test_nodeagent_memtest.py pins, by this copy."""
    w = ref_words(12346, 7)
    assert (int(w[2 * 12345]), int(w[2 * 12345 + 1])) == (0x1F6622B40CB38E42, 0xF34C71BDE099DD4B)
    w = ref_words(2, 0)
    assert (int(w[0]), int(w[1])) == (0, M64)
    assert (int(w[2]), int(w[3])) == (0x5692161D100B05E5, 0xEFF4FA1AA96DE9E2)


# ---------------------------------------------------------------------------
# CPU tests: argument errors, ahead of any HIP call
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


def test_library_exports_copy_run(cpu_agent):
    assert hasattr(cpu_agent.lib, "na_copy_run")


# never followed: every call below is refused before the pointers are used
SRC, DST = 1 << 40, (1 << 40) + (1 << 30)

COPY_RUN_ERRORS = [
    # (src, dst, bytes, workgroups, threads), what the message must name
    ((0, DST, 64, 1, 64), "src (nil)"),
    ((SRC, 0, 64, 1, 64), "dst (nil)"),
    ((SRC + 8, DST, 64, 1, 64), f"src {SRC + 8:#x}"),
    ((SRC, DST + 4, 64, 1, 64), f"dst {DST + 4:#x}"),
    ((SRC, DST, 0, 1, 64), "bytes (0)"),
    ((SRC, DST, -16, 1, 64), "bytes (-16)"),
    ((SRC, DST, 24, 1, 64), "bytes (24)"),
    ((SRC, DST, (1 << 35) + 8, 0, 0), f"bytes ({(1 << 35) + 8})"),
    ((SRC, DST, 64, 1, 32), "threads (32)"),
    ((SRC, DST, 64, 1, 96), "threads (96)"),
    ((SRC, DST, 64, 1, 1088), "threads (1088)"),
    ((SRC, DST, 64, 1, -64), "threads (-64)"),
    ((SRC, DST, 64, -1, 64), "workgroups (-1)"),
    ((SRC, DST, 64, 65536, 64), "workgroups (65536)"),
    # overlaps: the same range, dst inside src's, src inside dst's; one byte
    ((SRC, SRC, 64, 1, 64), "overlap"),
    ((SRC, SRC + 48, 64, 1, 64), "overlap"),
    ((SRC + 48, SRC, 64, 1, 64), "overlap"),
    ((SRC, SRC + (1 << 33), (1 << 33) + 16, 0, 0), "overlap"),
]


@pytest.mark.parametrize("args,names", COPY_RUN_ERRORS)
def test_copy_run_argument_errors_before_any_hip_call(cpu_agent, args, names):
    assert cpu_agent.copy_run(0, *args) == nodeagent.NA_ERR_ARG, args
    err = cpu_agent._err()
    assert err.startswith("na_copy_run: ") and names in err, err


PROBES = ["na_hbm_bandwidth", "na_sdma_bandwidth", "na_p2p_bandwidth"]


def _probe(lib, name, bytes_, iters, gbs, devs=(0, 1)):
    fn = getattr(lib, name)
    if name == "na_p2p_bandwidth":
        return fn(devs[0], devs[1], bytes_, iters, gbs)
    return fn(0, bytes_, iters, gbs)


@pytest.mark.parametrize("name", PROBES)
def test_probe_argument_errors_before_any_hip_call(cpu_agent, name):
    lib = cpu_agent.lib
    out = ctypes.c_double(-1.0)
    for bytes_, iters, gbs, names in [
        (15, 10, ctypes.byref(out), "bytes >= 16 (got 15)"),
        (0, 10, ctypes.byref(out), "bytes >= 16 (got 0)"),
        (-(1 << 30), 10, ctypes.byref(out), f"bytes >= 16 (got {-(1 << 30)})"),
        (1 << 20, 0, ctypes.byref(out), "iters >= 1 (got 0)"),
        (1 << 20, -3, ctypes.byref(out), "iters >= 1 (got -3)"),
        (1 << 20, 10, None, "(gbs (nil))"),
    ]:
        assert _probe(lib, name, bytes_, iters, gbs) == nodeagent.NA_ERR_ARG, (bytes_, iters)
        err = cpu_agent._err()
        assert err.startswith(name + ": ") and names in err, err
    assert out.value == -1.0  # and no figure was written


def test_p2p_argument_errors_before_any_hip_call(cpu_agent):
    out = ctypes.c_double(-1.0)
    for src, dst in [(0, 0), (3, 3), (-1, 0), (0, -1), (-2, -2)]:
        rc = _probe(cpu_agent.lib, "na_p2p_bandwidth", 1 << 20, 1, ctypes.byref(out), (src, dst))
        assert rc == nodeagent.NA_ERR_ARG, (src, dst)
        err = cpu_agent._err()
        assert err.startswith("na_p2p_bandwidth: ") and f"src {src}, dst {dst}" in err, err
    buf = (ctypes.c_int * 4)()
    for n, ptr, names in [(0, buf, "n >= 1 (got 0)"), (-8, buf, "n >= 1 (got -8)"),
                          (2, None, "(out (nil))")]:
        assert cpu_agent.lib.na_p2p_matrix(n, ptr) == nodeagent.NA_ERR_ARG, n
        err = cpu_agent._err()
        assert err.startswith("na_p2p_matrix: ") and names in err, err


def test_python_wrappers_raise_on_argument_errors(cpu_agent):
    with pytest.raises(nodeagent.NodeAgentError, match=r"na_hbm_bandwidth: .*iters >= 1 \(got 0\)"):
        cpu_agent.hbm_bandwidth(0, 1 << 20, iters=0)
    with pytest.raises(nodeagent.NodeAgentError, match=r"na_sdma_bandwidth: .*got -16"):
        cpu_agent.sdma_bandwidth(0, -16)
    with pytest.raises(nodeagent.NodeAgentError, match="na_p2p_bandwidth: .*src 1, dst 1"):
        cpu_agent.p2p_bandwidth(1, 1)
    with pytest.raises(nodeagent.NodeAgentError, match="na_p2p_matrix: "):
        cpu_agent.p2p_matrix(0)


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------

GUARD_VECS = 4
SRC_GUARD = 0x5A5AA5A5C3C33C3C
DST_GUARD = 0x0F0FF0F0A5A55A5A
DST_FILL = 0x7E57DEADBEEF0BAD  # what the destination holds before the copy
SEED = 7

# the probe's own shape, what 0 means to na_copy_run
PROBE_WORKGROUPS, PROBE_THREADS = 16384, 1024

# (workgroups G, threads B, vectors n). per = ceil(n / G) vectors go to each
# workgroup; a thread's unrolled pass takes vectors i, i+B, i+2B, i+3B.
CASES = (
    # tail loop only, fewer vectors than threads and just past them
    [(1, 64, n) for n in (1, 63, 64, 65)]
    # 255: tail loop only; 256: exactly one unrolled pass and no tail
    + [(1, 64, n) for n in (255, 256)]
    # a pass plus a one-thread tail; several passes plus a ragged tail
    + [(1, 64, n) for n in (257, 773)]
    # per = 1 and 2: workgroup 3 starts at n, and past n
    + [(4, 64, n) for n in (3, 5)]
    # last slice shorter, equal, and per = 257 with a short last slice
    + [(4, 64, n) for n in (1023, 1024, 1025)]
    # nothing divides anything
    + [(7, 128, 10007)]
    # the unrolled path at the probe's block size
    + [(2, 1024, 2 * 4096 + 1027)]
    # the probe's shape: almost every workgroup empty; per = 257 with most
    # threads idle; and the size the CLI test passes as --bw-bytes
    + [(0, 0, n) for n in (1, 16383, 16384, 16385, (1 << 22) + 7, 1 << 24)]
)
# up to here the comparison is numpy's on the host, which can say where
HOST_COMPARE_MAX_VECS = 1 << 16


def _signed(x):
    return x - (1 << 64) if x >= 1 << 63 else x


class Region:
    """``nvec`` vectors of device memory holding ``fill`` between guards of
    ``guard`` (64-bit words; the idea of test_nodeagent_memtest.py's)."""

    def __init__(self, nvec, guard, fill):
        self.nvec, self.guard = nvec, guard
        self.buf = torch.full(
            (2 * (nvec + 2 * GUARD_VECS),), _signed(guard), dtype=torch.int64, device="cuda:0"
        )
        self.words = self.buf[2 * GUARD_VECS: 2 * (GUARD_VECS + nvec)]
        self.words.fill_(_signed(fill))
        self.ptr = self.buf.data_ptr() + 16 * GUARD_VECS
        self.bytes = 16 * nvec
        assert self.words.data_ptr() == self.ptr and self.ptr % 16 == 0

    def host(self):
        torch.cuda.synchronize()
        return self.words.cpu().numpy().view(np.uint64)

    def guards_intact(self):
        torch.cuda.synchronize()
        g = torch.cat([self.buf[: 2 * GUARD_VECS], self.buf[-2 * GUARD_VECS:]])
        return bool((g == _signed(self.guard)).all().item())


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


def _where(got, want, workgroups, nvec):
    """The first differing vector of two word arrays and the workgroup whose
    slice it lies in."""
    v = int(np.flatnonzero(got != want)[0]) // 2
    grid = workgroups or PROBE_WORKGROUPS
    per = -(-nvec // grid)
    return (f"first differing vector {v} of {nvec}: in the slice of workgroup {v // per} of "
            f"{grid} ({per} vectors each), got {int(got[2 * v]):#018x} {int(got[2 * v + 1]):#018x} "
            f"want {int(want[2 * v]):#018x} {int(want[2 * v + 1]):#018x}")


@pytest.mark.gpu
@pytest.mark.parametrize("workgroups,threads,nvec", CASES)
def test_gpu_copy_run_moves_every_vector_and_nothing_else(agent, workgroups, threads, nvec):
    src = Region(nvec, SRC_GUARD, 0)
    dst = Region(nvec, DST_GUARD, DST_FILL)
    torch.cuda.synchronize()
    assert agent.memtest_fill(0, src.ptr, src.bytes, SEED) == nodeagent.NA_OK, agent._err()
    small = nvec <= HOST_COMPARE_MAX_VECS
    before = ref_words(nvec, SEED) if small else src.words.clone()
    torch.cuda.synchronize()

    rc = agent.copy_run(0, src.ptr, dst.ptr, 16 * nvec, workgroups, threads)
    assert rc == nodeagent.NA_OK, agent._err()

    if small:
        got_src, got_dst = src.host(), dst.host()
        assert np.array_equal(got_src, before), \
            "source changed: " + _where(got_src, before, workgroups, nvec)
        assert np.array_equal(got_dst, before), _where(got_dst, before, workgroups, nvec)
    else:
        torch.cuda.synchronize()
        assert torch.equal(src.words, before), "source changed"
        assert torch.equal(dst.words, before), "destination differs from the source"
    assert dst.guards_intact(), "the copy wrote outside the destination"
    assert src.guards_intact(), "the source's guards changed"


@pytest.mark.gpu
@pytest.mark.parametrize("upwards", [True, False])
def test_gpu_copy_run_takes_adjacent_ranges_and_the_ends_of_its_range(agent, upwards):
    """Ranges that touch do not overlap: one half of a region onto the other,
    at the largest grid with the smallest block, and back at the largest
    block."""
    nvec = 1000
    both = Region(2 * nvec, SRC_GUARD, DST_FILL)
    lo, hi = both.ptr, both.ptr + 16 * nvec
    src, dst = (lo, hi) if upwards else (hi, lo)
    torch.cuda.synchronize()
    assert agent.memtest_fill(0, src, 16 * nvec, SEED) == nodeagent.NA_OK, agent._err()
    workgroups, threads = (65535, 64) if upwards else (3, 1024)
    rc = agent.copy_run(0, src, dst, 16 * nvec, workgroups, threads)
    assert rc == nodeagent.NA_OK, agent._err()
    want = ref_words(nvec, SEED)
    got = both.host()
    assert np.array_equal(got[: 2 * nvec], want), _where(got[: 2 * nvec], want, workgroups, nvec)
    assert np.array_equal(got[2 * nvec:], want), _where(got[2 * nvec:], want, workgroups, nvec)
    assert both.guards_intact()


@pytest.mark.gpu
def test_gpu_copy_run_argument_errors_launch_nothing(agent):
    src = Region(64, SRC_GUARD, 0)
    dst = Region(64, DST_GUARD, DST_FILL)
    torch.cuda.synchronize()
    for args in [(src.ptr + 8, dst.ptr, 64, 1, 64), (src.ptr, dst.ptr, 24, 1, 64),
                 (src.ptr, dst.ptr, 64, 1, 100), (src.ptr, dst.ptr, 64, 70000, 64),
                 (dst.ptr, dst.ptr + 16, 64, 1, 64)]:
        assert agent.copy_run(0, *args) == nodeagent.NA_ERR_ARG, args
    assert np.array_equal(dst.host(), np.full(128, DST_FILL, dtype=np.uint64))
    assert dst.guards_intact() and src.guards_intact()


@pytest.mark.gpu
@pytest.mark.parametrize("probe", ["hbm_bandwidth", "sdma_bandwidth"])
def test_gpu_probe_verifies_a_size_that_is_no_multiple_of_16(agent, probe):
    """(1 << 20) + 8 bytes, one timed copy: the whole vectors are verified and
    the call succeeds (a failure would raise with the NA_ERR_VERIFY message)."""
    torch.cuda.synchronize()
    out = ctypes.c_double(0)
    rc = getattr(agent.lib, "na_" + probe)(0, (1 << 20) + 8, 1, ctypes.byref(out))
    assert rc == nodeagent.NA_OK, agent._err()
    assert out.value > 0
    # the smallest size there is
    assert getattr(agent, probe)(0, 16, 1) > 0


@pytest.mark.gpu
def test_gpu_p2p_bandwidth_verifies_on_the_destination_device(agent):
    if agent.device_count() < 2:
        pytest.skip("p2p_bandwidth needs device_count() >= 2")
    torch.cuda.synchronize()
    out = ctypes.c_double(0)
    rc = agent.lib.na_p2p_bandwidth(0, 1, (1 << 20) + 8, 1, ctypes.byref(out))
    assert rc == nodeagent.NA_OK, agent._err()
    assert out.value > 0
    assert agent.p2p_bandwidth(0, 1) > 0
