"""Single-wave MFMA checks of the node agent (na_mfma_check_run /
na_mfma_check_verify, nodeagent/agent.hip and nodeagent/mfma_frag.h).

The reference for every kind is the numpy copy of the operand formulas
below, written from the specification and independent of the kernel and of
the host verify, and pinned by known answers:

  tile_a(i, k) = (i*31 + k*7) % 7 - 3      tile_b(k, j) = (k*13 + j*3) % 5 - 2
  tile kinds:    D = A·B, row-major; the MX kinds take k modulo 64 and the
                 second of them doubles D (E8M0 scale 2.0 on A)
  uniform kinds: every word is 2*K*1.5*2.0 (two chained MFMAs on alpha = 1.5,
                 beta = 2.0): 24 for f32 (K = 4), 192 for bf16 and fp8 (K = 32)

CPU: the verify on the expected words, on words with one value changed (the
failure branch and its message), on the wrong-arch fill, and argument errors
of both functions. GPU (@pytest.mark.gpu, device 0): one wave per kind,
words equal to the reference exactly. Only HOST data is corrupted; nothing on
the GPU is provoked.
"""
import ctypes
import os
import re

import numpy as np
import pytest

# torch first, before any test loads the agent library: see the note at the
# top of test_nodeagent_memtest.py (one HIP runtime per process — torch's).
try:
    import torch
except ImportError:  # CPU-only environment: the GPU tests cannot run there
    torch = None

from gpu_provisioner_amd import nodeagent


def _ensure_lib():
    import __graft_entry__ as g

    if not os.path.exists(g.LIB_PATH):
        g.build()
    return g.LIB_PATH


# ---------------------------------------------------------------------------
# numpy reference of the specification
# ---------------------------------------------------------------------------


def ref_tile(mn, k_len, kmod=None, mult=1):
    """D[mn][mn] = A[mn][k_len] · B[k_len][mn] as int64."""
    i = np.arange(mn, dtype=np.int64)[:, None]
    k = np.arange(k_len, dtype=np.int64)
    if kmod:
        k = k % kmod
    a = (i * 31 + k[None, :] * 7) % 7 - 3
    b = (k[:, None] * 13 + i.T * 3) % 5 - 2
    return (a @ b) * mult


# kind -> (message prefix, expected D or uniform constant, word dtype)
def _kinds():
    t32 = ref_tile(16, 32)
    return {
        "f32_uniform": ("mfma selftest", 2 * 4 * 1.5 * 2.0, np.float32),
        "bf16_uniform": ("mfma-bf16 selftest", 2 * 32 * 1.5 * 2.0, np.float32),
        "fp8_uniform": ("mfma-fp8 selftest", 2 * 32 * 1.5 * 2.0, np.float32),
        "bf16_tile": ("mfma bf16 tile", t32, np.float32),
        "f16_tile": ("mfma f16 tile", t32, np.float32),
        "fp8_tile": ("mfma fp8 tile", t32, np.float32),
        "i8_tile": ("mfma i8 tile", ref_tile(16, 64), np.int32),
        "bf16_tile32": ("mfma bf16 32x32 tile", ref_tile(32, 16), np.float32),
        "mx_tile": ("mfma mx tile (scale 1x)", ref_tile(16, 128, kmod=64), np.float32),
        "mx_tile_x2": ("mfma mx tile (scale 2x)", ref_tile(16, 128, kmod=64, mult=2), np.float32),
    }


KINDS = _kinds()
UNIFORM = ("f32_uniform", "bf16_uniform", "fp8_uniform")


def expected_words(kind):
    """The kind's words as the run leaves them: D row-major, or 256 times
    the uniform constant."""
    _, want, dtype = KINDS[kind]
    if kind in UNIFORM:
        return np.full(256, want, dtype=dtype)
    return want.astype(dtype).ravel()


def _where(kind, pos):
    """How the failure message names word ``pos``."""
    if kind in UNIFORM:
        return f"elem {pos}"
    mn = KINDS[kind][1].shape[0]
    return f"D[{pos // mn}][{pos % mn}]"


def _ptr(words):
    return words.ctypes.data_as(ctypes.c_void_p)


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------


def test_kind_codes_mirror_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "nodeagent", "mfma_frag.h")) as f:
        body = re.search(r"enum \{\s*NA_MFMA_F32_UNIFORM = 0,(.*?)NA_MFMA_KINDS", f.read(), re.S)
    names = ["f32_uniform"] + [n.lower() for n in re.findall(r"NA_MFMA_(\w+),", body.group(1))]
    assert nodeagent.MFMA_CHECK_KINDS == {n: i for i, n in enumerate(names)}
    assert set(KINDS) == set(nodeagent.MFMA_CHECK_KINDS)


def test_reference_known_answers():
    d = KINDS["bf16_tile"][1]
    assert (d[0, 0], d[3, 5], d[15, 15], d.sum(), np.abs(d).max()) == (3, 1, 0, 3, 6)
    d = KINDS["i8_tile"][1]
    assert (d[0, 0], d[3, 5], d.sum(), np.abs(d).max()) == (0, 0, 0, 6)
    d = KINDS["bf16_tile32"][1]
    assert d.shape == (32, 32)
    assert (d[0, 0], d[3, 5], d[31, 31], d.sum()) == (6, 2, -1, 1)
    d = KINDS["mx_tile"][1]
    assert (d.sum(), np.abs(d).max()) == (0, 12)
    assert np.array_equal(KINDS["mx_tile_x2"][1], 2 * d) and np.abs(2 * d).max() == 24
    assert [KINDS[k][1] for k in UNIFORM] == [24.0, 192.0, 192.0]


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


def test_library_exports_mfma_check_symbols(cpu_agent):
    for sym in ("na_mfma_check_run", "na_mfma_check_verify"):
        assert hasattr(cpu_agent.lib, sym), f"missing symbol {sym}"


@pytest.mark.parametrize("kind", list(KINDS))
def test_verify_accepts_expected_words(cpu_agent, kind):
    words = expected_words(kind)
    as_run_returns = (ctypes.c_uint32 * len(words)).from_buffer(words)
    assert cpu_agent.mfma_check_verify(kind, as_run_returns) == nodeagent.NA_OK
    # a longer buffer is fine: only the kind's own words are read
    longer = np.concatenate([words, np.full(8, -1, dtype=words.dtype)])
    rc = cpu_agent.lib.na_mfma_check_verify(nodeagent.MFMA_CHECK_KINDS[kind], _ptr(longer),
                                            len(longer))
    assert rc == nodeagent.NA_OK


@pytest.mark.parametrize("kind", list(KINDS))
def test_verify_names_one_changed_word(cpu_agent, kind):
    label, _, dtype = KINDS[kind]
    good = expected_words(kind)
    code = nodeagent.MFMA_CHECK_KINDS[kind]
    for pos in (0, len(good) // 2 + 3, len(good) - 1):
        words = good.copy()
        words[pos] += 5 if dtype == np.int32 else 0.5
        rc = cpu_agent.lib.na_mfma_check_verify(code, _ptr(words), len(words))
        assert rc == nodeagent.NA_ERR_VERIFY, (kind, pos)
        if dtype == np.int32:
            want = f"{label}: {_where(kind, pos)} got {words[pos]:d} want {good[pos]:d}"
        else:
            want = f"{label}: {_where(kind, pos)} got {words[pos]:g} want {good[pos]:g}"
        assert cpu_agent._err() == want
    # the first of several bad words is the one named
    words = good.copy()
    words[[7, 200]] += 1
    assert cpu_agent.lib.na_mfma_check_verify(code, _ptr(words), len(words)) \
        == nodeagent.NA_ERR_VERIFY
    assert f"{label}: {_where(kind, 7)} got " in cpu_agent._err()


def test_verify_compares_by_value_not_bit_pattern(cpu_agent):
    words = expected_words("bf16_tile")
    assert words[255] == 0
    words[255] = -0.0  # another bit pattern of the same value
    code = nodeagent.MFMA_CHECK_KINDS["bf16_tile"]
    assert cpu_agent.lib.na_mfma_check_verify(code, _ptr(words), 256) == nodeagent.NA_OK
    words[255] = np.nan
    assert cpu_agent.lib.na_mfma_check_verify(code, _ptr(words), 256) == nodeagent.NA_ERR_VERIFY


@pytest.mark.parametrize("kind", list(KINDS))
def test_verify_rejects_the_wrong_arch_fill(cpu_agent, kind):
    words = np.full(len(expected_words(kind)), -1, dtype=KINDS[kind][2])
    rc = cpu_agent.lib.na_mfma_check_verify(nodeagent.MFMA_CHECK_KINDS[kind], _ptr(words),
                                            len(words))
    assert rc == nodeagent.NA_ERR_VERIFY
    assert f"{KINDS[kind][0]}: {_where(kind, 0)} got -1 want " in cpu_agent._err()


def test_argument_errors_before_any_hip_call(cpu_agent):
    """Both functions, with no GPU present: unknown kind, null pointer,
    short buffer."""
    lib = cpu_agent.lib
    buf = np.zeros(1024, dtype=np.uint32)
    n_kinds = len(nodeagent.MFMA_CHECK_KINDS)
    for kind, ptr, n in [(-1, _ptr(buf), 1024), (n_kinds, _ptr(buf), 1024), (0, None, 1024),
                         (0, _ptr(buf), 255), (7, _ptr(buf), 1023), (9, _ptr(buf), 0),
                         (3, _ptr(buf), -1)]:
        assert lib.na_mfma_check_run(0, kind, ptr, n) == nodeagent.NA_ERR_ARG, (kind, n)
        assert cpu_agent._err().startswith("na_mfma_check_run: ")
        assert lib.na_mfma_check_verify(kind, ptr, n) == nodeagent.NA_ERR_ARG, (kind, n)
        assert cpu_agent._err().startswith("na_mfma_check_verify: ")
    with pytest.raises(KeyError):
        cpu_agent.mfma_check_verify("fp4_tile", (ctypes.c_uint32 * 256)())


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def agent():
    _ensure_lib()
    torch.cuda.init()
    return nodeagent.NodeAgent()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_gpu_words_match_reference(agent, kind):
    torch.cuda.synchronize()
    words = agent.mfma_check_run(0, kind)
    want = expected_words(kind)
    got = np.frombuffer(words, dtype=want.dtype, count=len(want))
    assert np.array_equal(got, want), f"{kind}: first mismatch at {np.argmax(got != want)}"
    assert agent.mfma_check_verify(kind, words) == nodeagent.NA_OK, agent._err()
