"""Single-wave MX checks of the node agent (na_mx_check_run /
na_mx_check_verify, nodeagent/agent.hip, nodeagent/mfma_frag.h and
nodeagent/mx_formats.h): v_mfma_scale_f32_{16x16x128,32x32x64}_f8f6f4 in
every operand format, with per-lane scales and every scale byte select.

The reference for everything is the numpy code below, written from the
specification and independent of the header, the kernels and the host verify,
and pinned by known answers.

Formats (OCP MX; code = the instruction's cbsz / blgp value):
  0 E4M3  s eeee mmm  bias 7   S.1111.111 is NaN, no inf
  1 E5M2  s eeeee mm  bias 15  IEEE-like: e = 31 is inf (m = 0) or NaN
  2 E2M3  s ee mmm    bias 1   no inf / NaN
  3 E3M2  s eee mm    bias 3   no inf / NaN
  4 E2M1  s ee m      bias 1   no inf / NaN
  all with subnormals: e = 0 is m * 2^(1 - bias - mantissa bits)
Packing: element i of a 32-element fragment at bit i * width, little-endian
across 32-bit words: 8, 6 or 4 words.

Tile kinds (both operands vary in k; blk = k // 32; E8M0 byte = 127 + e):
  a(i,k) = ((i*5 + k*3 + (k>>4)) % 7) - 3    b(k,j) = ((k*2 + j*3 + (k>>5)) % 5) - 2
  ea(i,blk) = ((i + 2*blk) % 4) - 1          eb(blk,j) = ((j*3 + blk) % 3) - 1
  D[i][j] = sum_blk 2^(ea+eb) * sum_{k in blk} a(i,k) * b(k,j)
Code-point kinds (n = 16 for fp4, 64 for fp6 and bf6):
  A[i][k] = code (i*37 + k*11) % n; B[k][j] = 1.0 where k % 16 == j, else 0;
  D[i][j] = sum_{m<8} decode(code(i, j + 16m))

CPU: decoders and packer of the library against numpy, the known answers,
the kind codes, the verify on the expected words and on words with one value
changed, the wrong-arch fill, and argument errors. GPU (@pytest.mark.gpu,
device 0): one wave per kind, words equal to the reference exactly. Only HOST
data is corrupted; nothing on the GPU is provoked.
"""
import ctypes
import math
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

# name -> (code, exponent bits, mantissa bits, bias)
FORMATS = {
    "e4m3": (0, 4, 3, 7), "e5m2": (1, 5, 2, 15), "e2m3": (2, 2, 3, 1), "e3m2": (3, 3, 2, 3),
    "e2m1": (4, 2, 1, 1),
}


def ref_decode(fmt, code):
    _, ebits, mbits, bias = FORMATS[fmt]
    sign = -1.0 if code >> (ebits + mbits) else 1.0
    e = (code >> mbits) & ((1 << ebits) - 1)
    m = code & ((1 << mbits) - 1)
    if fmt == "e4m3" and e == 15 and m == 7:
        return math.nan
    if fmt == "e5m2" and e == 31:
        return math.nan if m else sign * math.inf
    if e == 0:
        return sign * m * 2.0 ** (1 - bias - mbits)
    return sign * (1 + m / (1 << mbits)) * 2.0 ** (e - bias)


def ref_pack(width, codes):
    """Each run of 32 codes as one little-endian integer of 32 * width bits,
    cut into 32-bit words."""
    words = []
    for f in range(0, len(codes), 32):
        value = sum(int(c) << (i * width) for i, c in enumerate(codes[f:f + 32]))
        words += [(value >> (32 * j)) & 0xFFFFFFFF for j in range(width)]
    return words


def ref_tile_operands(mn, k_len):
    i = np.arange(mn, dtype=np.int64)[:, None]
    k = np.arange(k_len, dtype=np.int64)
    a = (i * 5 + k[None, :] * 3 + (k[None, :] >> 4)) % 7 - 3
    b = (k[:, None] * 2 + i.T * 3 + (k[:, None] >> 5)) % 5 - 2
    blk = np.arange(k_len // 32, dtype=np.int64)
    ea = (i + 2 * blk[None, :]) % 4 - 1           # [i][blk]
    eb = (i.T * 3 + blk[:, None]) % 3 - 1         # [blk][j]
    return a, b, ea, eb


def ref_tile(mn, k_len):
    """D[mn][mn] as float64 (every value a multiple of 1/4 below 2^13)."""
    a, b, ea, eb = ref_tile_operands(mn, k_len)
    d = np.zeros((mn, mn))
    for blk in range(k_len // 32):
        ks = slice(32 * blk, 32 * blk + 32)
        d += (a[:, ks] @ b[ks, :]) * 2.0 ** (ea[:, blk][:, None] + eb[blk][None, :])
    return d


def ref_codes(fmt):
    n = 1 << (1 + FORMATS[fmt][1] + FORMATS[fmt][2])
    d = np.zeros((16, 16))
    for i in range(16):
        for j in range(16):
            d[i, j] = sum(ref_decode(fmt, (i * 37 + (j + 16 * m) * 11) % n) for m in range(8))
    return d


# kind -> (message prefix, expected D)
def _kinds():
    t16, t32 = ref_tile(16, 128), ref_tile(32, 64)
    return {
        "fp4": ("mx fp4 tile", t16),
        "fp6": ("mx fp6 tile", t16),
        "bf6": ("mx bf6 tile", t16),
        "bf8": ("mx bf8 tile", t16),
        "fp8_fp4": ("mx fp8 x fp4 tile", t16),
        "fp4_32": ("mx fp4 32x32 tile", t32),
        "fp4_codes": ("mx fp4 codes", ref_codes("e2m1")),
        "fp6_codes": ("mx fp6 codes", ref_codes("e2m3")),
        "bf6_codes": ("mx bf6 codes", ref_codes("e3m2")),
    }


KINDS = _kinds()


def expected_words(kind):
    """The kind's words as the run leaves them: D row-major in float32."""
    d = KINDS[kind][1]
    words = d.astype(np.float32).ravel()
    assert np.array_equal(words.astype(np.float64), d.ravel())  # exact in f32
    return words


def _where(kind, pos):
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
        body = re.search(r"enum \{\s*NA_MX_FP4 = 0,(.*?)NA_MX_KINDS", f.read(), re.S)
    names = ["fp4"] + [n.lower() for n in re.findall(r"NA_MX_(\w+),", body.group(1))]
    assert nodeagent.MX_CHECK_KINDS == {n: i for i, n in enumerate(names)}
    assert set(KINDS) == set(nodeagent.MX_CHECK_KINDS)
    assert {k: v[0] for k, v in FORMATS.items()} == nodeagent.MX_FORMATS


def test_reference_decode_known_values():
    assert [ref_decode("e2m1", c) for c in range(8)] == [0, 0.5, 1, 1.5, 2, 3, 4, 6]
    assert [ref_decode("e2m1", c) for c in range(8, 16)] == [-0.0, -0.5, -1, -1.5, -2, -3, -4, -6]
    assert (ref_decode("e2m3", 0x01), ref_decode("e2m3", 0x1F), ref_decode("e2m3", 0x3F)) \
        == (0.125, 7.5, -7.5)
    assert (ref_decode("e3m2", 0x01), ref_decode("e3m2", 0x1F), ref_decode("e3m2", 0x0C)) \
        == (0.0625, 28.0, 1.0)
    assert (ref_decode("e4m3", 0x7E), ref_decode("e4m3", 0x38), ref_decode("e4m3", 0x01)) \
        == (448.0, 1.0, 2.0 ** -9)
    assert (ref_decode("e5m2", 0x7B), ref_decode("e5m2", 0x3C), ref_decode("e5m2", 0x01)) \
        == (57344.0, 1.0, 2.0 ** -16)
    assert ref_decode("e5m2", 0x7C) == math.inf and ref_decode("e5m2", 0xFC) == -math.inf
    assert math.isnan(ref_decode("e5m2", 0x7D)) and math.isnan(ref_decode("e4m3", 0xFF))


def test_reference_known_answers():
    """Computed from the formulas with numpy, not on a GPU."""
    d = KINDS["fp4"][1]
    assert (d[0, 0], d[3, 5], d[15, 15], d.sum(), np.abs(d).max()) == (59.5, 138, -34.5, 133, 218.5)
    a, b, _, _ = ref_tile_operands(16, 128)
    u = a @ b  # the unscaled product
    assert (u[0, 0], u.sum(), np.abs(u).max()) == (56, 44, 76)
    d = KINDS["fp4_32"][1]
    assert d.shape == (32, 32)
    assert (d[0, 0], d[3, 5], d[31, 31], d.sum(), np.abs(d).max()) == (31.5, 36, -57, 22.5, 85.5)
    for kind in ("fp4", "fp4_32"):
        d = KINDS[kind][1]
        assert np.array_equal(d * 4, np.round(d * 4)) and np.abs(d).max() < 2 ** 13
    # both operands vary in k: no two neighbouring k carry the same data
    assert all(not np.array_equal(a[:, k], a[:, k + 1]) for k in range(127))
    assert all(not np.array_equal(b[k], b[k + 1]) for k in range(127))
    # every code of each sub-byte format is in every row of the code-point A
    for n in (16, 64):
        for i in range(16):
            assert {(i * 37 + k * 11) % n for k in range(128)} == set(range(n))
    assert np.abs(KINDS["bf6_codes"][1]).max() <= 224


@pytest.fixture(scope="module")
def cpu_agent():
    _ensure_lib()
    return nodeagent.NodeAgent()


def test_library_exports_mx_symbols(cpu_agent):
    for sym in ("na_mx_decode", "na_mx_pack", "na_mx_check_run", "na_mx_check_verify",
                "na_mx_checks"):
        assert hasattr(cpu_agent.lib, sym), f"missing symbol {sym}"


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_decode_matches_reference_for_every_code(cpu_agent, fmt):
    _, ebits, mbits, _ = FORMATS[fmt]
    n = 1 << (1 + ebits + mbits)
    assert n == 1 << nodeagent.MX_FORMAT_BITS[fmt]
    for code in range(n):
        got, want = cpu_agent.mx_decode(fmt, code), ref_decode(fmt, code)
        if math.isnan(want):
            assert math.isnan(got), (fmt, code)
        else:  # inf compares equal to inf; the sign of zero counts too
            assert got == want and math.copysign(1, got) == math.copysign(1, want), (fmt, code)
    out = ctypes.c_float(0)
    for code in (-1, n):
        assert cpu_agent.lib.na_mx_decode(FORMATS[fmt][0], code, ctypes.byref(out)) \
            == nodeagent.NA_ERR_ARG
    assert cpu_agent.lib.na_mx_decode(FORMATS[fmt][0], 0, None) == nodeagent.NA_ERR_ARG


def test_decode_rejects_unknown_formats(cpu_agent):
    out = ctypes.c_float(0)
    for fmt in (-1, 5):
        assert cpu_agent.lib.na_mx_decode(fmt, 0, ctypes.byref(out)) == nodeagent.NA_ERR_ARG
        assert cpu_agent._err().startswith("na_mx_decode: ")


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_pack_matches_reference(cpu_agent, fmt):
    width = nodeagent.MX_FORMAT_BITS[fmt]
    rng = np.random.default_rng(width)
    for n in (32, 96):
        codes = rng.integers(0, 1 << width, size=n)
        assert cpu_agent.mx_pack(fmt, list(codes)) == ref_pack(width, codes)
    # one element at a time, all bits set: every position, the 6-bit elements
    # that straddle two words (5, 10, 15, ...) included
    for i in range(32):
        codes = [0] * 32
        codes[i] = (1 << width) - 1
        assert cpu_agent.mx_pack(fmt, codes) == ref_pack(width, codes), (fmt, i)
    if width == 6:
        assert ref_pack(6, [0] * 5 + [0x3F] + [0] * 26)[:2] == [0xC0000000, 0xF]


def test_pack_argument_errors(cpu_agent):
    lib = cpu_agent.lib
    codes = (ctypes.c_int * 64)()
    words = (ctypes.c_uint32 * 16)()
    for fmt, c, n, w, n_words in [(5, codes, 32, words, 16), (-1, codes, 32, words, 16),
                                  (4, codes, 0, words, 16), (4, codes, 33, words, 16),
                                  (4, codes, -32, words, 16), (4, None, 32, words, 16),
                                  (4, codes, 32, None, 16), (4, codes, 32, words, 3),
                                  (2, codes, 64, words, 11), (0, codes, 64, words, 15)]:
        assert lib.na_mx_pack(fmt, c, n, w, n_words) == nodeagent.NA_ERR_ARG, (fmt, n, n_words)
        assert cpu_agent._err().startswith("na_mx_pack: ")
    assert lib.na_mx_pack(2, codes, 64, words, 12) == nodeagent.NA_OK
    codes[7] = 16  # not a 4-bit code
    assert lib.na_mx_pack(4, codes, 32, words, 16) == nodeagent.NA_ERR_ARG
    codes[7] = -1
    assert lib.na_mx_pack(4, codes, 32, words, 16) == nodeagent.NA_ERR_ARG


@pytest.mark.parametrize("kind", list(KINDS))
def test_verify_accepts_expected_words(cpu_agent, kind):
    words = expected_words(kind)
    as_run_returns = (ctypes.c_uint32 * len(words)).from_buffer(words)
    assert cpu_agent.mx_check_verify(kind, as_run_returns) == nodeagent.NA_OK, cpu_agent._err()
    # a longer buffer is fine: only the kind's own words are read
    longer = np.concatenate([words, np.full(8, -1, dtype=words.dtype)])
    rc = cpu_agent.lib.na_mx_check_verify(nodeagent.MX_CHECK_KINDS[kind], _ptr(longer),
                                          len(longer))
    assert rc == nodeagent.NA_OK


@pytest.mark.parametrize("kind", list(KINDS))
def test_verify_names_one_changed_word(cpu_agent, kind):
    label = KINDS[kind][0]
    good = expected_words(kind)
    code = nodeagent.MX_CHECK_KINDS[kind]
    for pos in (0, len(good) // 2 + 3, len(good) - 1):
        words = good.copy()
        words[pos] += 0.25
        rc = cpu_agent.lib.na_mx_check_verify(code, _ptr(words), len(words))
        assert rc == nodeagent.NA_ERR_VERIFY, (kind, pos)
        want = f"{label}: {_where(kind, pos)} got {words[pos]:g} want {good[pos]:g}"
        assert cpu_agent._err() == want
    # the first of several bad words is the one named
    words = good.copy()
    words[[7, 200]] += 1
    assert cpu_agent.lib.na_mx_check_verify(code, _ptr(words), len(words)) \
        == nodeagent.NA_ERR_VERIFY
    assert f"{label}: {_where(kind, 7)} got " in cpu_agent._err()


@pytest.mark.parametrize("kind", list(KINDS))
def test_verify_rejects_the_wrong_arch_fill(cpu_agent, kind):
    words = np.full(len(expected_words(kind)), -1, dtype=np.float32)
    rc = cpu_agent.lib.na_mx_check_verify(nodeagent.MX_CHECK_KINDS[kind], _ptr(words), len(words))
    assert rc == nodeagent.NA_ERR_VERIFY
    assert f"{KINDS[kind][0]}: {_where(kind, 0)} got -1 want " in cpu_agent._err()


def test_argument_errors_before_any_hip_call(cpu_agent):
    """Both functions, with no GPU present: unknown kind, null pointer,
    short buffer."""
    lib = cpu_agent.lib
    buf = np.zeros(1024, dtype=np.uint32)
    n_kinds = len(nodeagent.MX_CHECK_KINDS)
    for kind, ptr, n in [(-1, _ptr(buf), 1024), (n_kinds, _ptr(buf), 1024), (0, None, 1024),
                         (0, _ptr(buf), 255), (5, _ptr(buf), 1023), (8, _ptr(buf), 0),
                         (3, _ptr(buf), -1)]:
        assert lib.na_mx_check_run(0, kind, ptr, n) == nodeagent.NA_ERR_ARG, (kind, n)
        assert cpu_agent._err().startswith("na_mx_check_run: ")
        assert lib.na_mx_check_verify(kind, ptr, n) == nodeagent.NA_ERR_ARG, (kind, n)
        assert cpu_agent._err().startswith("na_mx_check_verify: ")
    with pytest.raises(KeyError):
        cpu_agent.mx_check_verify("fp4_tile", (ctypes.c_uint32 * 256)())
    # the existing kind spaces are as they were
    assert len(nodeagent.MFMA_CHECK_KINDS) == 10 and nodeagent.MFMA_SWEEP_DTYPES == {
        "bf16": 0, "fp8": 1}


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
    words = agent.mx_check_run(0, kind)
    want = expected_words(kind)
    got = np.frombuffer(words, dtype=np.float32, count=len(want))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (
        f"{kind}: {bad.size} of {len(want)} words differ, first {_where(kind, bad[0])} "
        f"got {got[bad[0]]:g} want {want[bad[0]]:g}")
    assert agent.mx_check_verify(kind, words) == nodeagent.NA_OK, agent._err()


@pytest.mark.gpu
def test_gpu_mx_checks_all_kinds(agent):
    torch.cuda.synchronize()
    assert agent.mx_checks(0), agent._err()
