"""Python binding + CLI for the MI355X node agent (nodeagent/agent.hip).

Runs on provisioned nodes (DaemonSet) to validate the GPU stack before the
node is trusted, and feeds the node.health repair policy with on-node
evidence. Fails LOUDLY if the native library is missing on a GPU machine —
there is no eager/python fallback for the hardware checks.

CLI: ``python -m gpu_provisioner_amd.nodeagent [--json] [--expect-gpus N]
[--memtest-bytes N] [--mfma-sweep] [--mx-checks] [--mx-sweep] [--lds-sweep]
[--cache-sweep] [--valu-sweep] [--load-sweep]``
Exit 0 = healthy, 1 = unhealthy/degraded, 2 = agent error.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
from dataclasses import asdict, dataclass, field, fields

_LIB_NAME = "libmi355x_nodeagent.so"
_SEARCH_PATHS = (
    os.path.join(os.path.dirname(__file__), "_native", _LIB_NAME),
    os.path.join(os.path.dirname(__file__), "..", "nodeagent", _LIB_NAME),
)

EXPECTED_ARCH = "gfx950"
EXPECTED_HBM_GB = 288
# healthy-node floors (MI355X: 8 TB/s HBM peak; the contiguous-chunk nt
# copy probe measures ~5.7 TB/s on healthy silicon — floor leaves margin
# for box-to-box variance; xGMI 7 links x ~153 GB/s guide values)
MIN_HBM_BW_GBS = 4800.0
MIN_XGMI_BW_GBS = 30.0
# D2D copy path (SDMA/blit — the hardware RCCL's transports lean on);
# measured ~4.9 TB/s on healthy silicon (profiles/), floor leaves margin
MIN_SDMA_BW_GBS = 3000.0

# C ABI return codes (nodeagent/nodeagent.h: NA_OK .. NA_ERR_ARG)
NA_OK = 0
NA_ERR_HIP = -1
NA_ERR_VERIFY = -2
NA_ERR_ARG = -3

# HBM data-integrity test. Seed 0 would make vector 0 all-zeros/all-ones, so
# the default is non-zero ("MI355XMT"); round r uses seed + r.
DEFAULT_MEMTEST_SEED = 0x4D493335_35584D54
NO_BAD_OFFSET = (1 << 64) - 1
# the agent never asks for more than this share of what the device reports
# free: the node may be running workloads
MEMTEST_FREE_FRACTION_PCT = 90

# Chip-wide matrix-core sweep. The default seed is "MI355XMS"; dtype codes
# are those of nodeagent/mfmasweep.h.
DEFAULT_MFMA_SWEEP_SEED = 0x4D493335_35584D53
MFMA_SWEEP_DTYPES = {"bf16": 0, "fp8": 1}
MFMA_SWEEP_WAVES_PER_WG = 4  # nodeagent/nodeagent.h: NA_SWEEP_WAVES_PER_WG
# nodeagent/nodeagent.h: NA_SWEEP_MAX_LISTED, the one limit of all three sweeps' lists
MFMA_SWEEP_MAX_LISTED = LDS_SWEEP_MAX_LISTED = VALU_SWEEP_MAX_LISTED = 8
NO_BAD_WAVE = (1 << 64) - 1
# bf16 floor of the default sweep: 0.70 x the 2282.1 TFLOP/s median measured
# on MI355X (profiles/mfma_sweep_mi355x.txt); the margin covers the 12 %
# device-to-device spread of MFMA-only loops. Integer operands held in
# registers clock higher than a random-data GEMM, so the figure is NOT
# comparable to GEMM benchmarks. 0 disables the floor.
MIN_MFMA_SWEEP_TFLOPS = 1597.5

# Single-wave MFMA checks: kind codes of nodeagent/mfma_frag.h. A kind yields
# 256 32-bit words (1024 for the 32x32 tile), int32 for i8, float32 otherwise.
MFMA_CHECK_KINDS = {
    "f32_uniform": 0, "bf16_uniform": 1, "fp8_uniform": 2, "bf16_tile": 3, "f16_tile": 4,
    "fp8_tile": 5, "i8_tile": 6, "bf16_tile32": 7, "mx_tile": 8, "mx_tile_x2": 9,
}
MFMA_CHECK_MAX_WORDS = 1024

# Single-wave MX checks (the block-scaled f8f6f4 instructions in every operand
# format): kind codes NA_MX_* of nodeagent/mfma_frag.h. A kind yields 256
# float32 words (1024 for the 32x32 tile).
MX_CHECK_KINDS = {
    "fp4": 0, "fp6": 1, "bf6": 2, "bf8": 3, "fp8_fp4": 4, "fp4_32": 5,
    "fp4_codes": 6, "fp6_codes": 7, "bf6_codes": 8,
}
# OCP MX element formats, coded as the instruction's cbsz / blgp
# (nodeagent/mx_formats.h), and their element widths in bits.
MX_FORMATS = {"e4m3": 0, "e5m2": 1, "e2m3": 2, "e3m2": 3, "e2m1": 4}
MX_FORMAT_BITS = {"e4m3": 8, "e5m2": 8, "e2m3": 6, "e3m2": 6, "e2m1": 4}

# Chip-wide MX sweep: the matrix-core sweep on the block-scaled 16x16x128
# instruction. The default seed is "MI355XMX".
DEFAULT_MX_SWEEP_SEED = 0x4D493335_35584D58
MX_SWEEP_FORMATS = {"fp4": 0, "fp6": 1}
# fp4 floor of the default MX sweep: 0.70 x the 7672.1 TFLOP/s median of five
# processes on MI355X (profiles/mx_sweep_mi355x.txt), the rule of the bf16
# floor above and with its caveat: not comparable to GEMM benchmarks.
# 0 disables the floor.
MIN_MX_SWEEP_TFLOPS = 5370.5

# Chip-wide LDS sweep (nodeagent/ldssweep.h). The default seed is "MI355XLS";
# a record carries one checksum per phase, in this order.
DEFAULT_LDS_SWEEP_SEED = 0x4D493335_35584C53
LDS_SWEEP_PHASES = ("b32", "b128", "dma16", "dma4", "dma12", "tr16", "atomic", "stream")
# nodeagent/nodeagent.h: NA_LDS_PHASES of them, NA_LDS_GRANULE, NA_LDS_MAX_BYTES
LDS_SWEEP_GRANULE = 4096  # lds_bytes is a multiple of this
LDS_SWEEP_MAX_BYTES = 160 * 1024
LDS_SWEEP_PEAK_BYTES_PER_CLK = 256  # what a CU's LDS delivers per clock: a ceiling, no floor
NO_BAD_WORKGROUP = (1 << 64) - 1
# Floor of the default sweep's chip-wide stream rate: 0.70 x the 117806.3 GB/s
# median of five processes on MI355X (profiles/lds_sweep_mi355x.txt; 195 of
# the LDS's 256 bytes per clock and CU). The device-to-device spread of LDS
# loops has not been measured; 0.70 is borrowed from the MFMA floor above.
# 0 disables the floor.
MIN_LDS_SWEEP_GBS = 82464.4

# Chip-wide cache sweep (nodeagent/cachesweep.h). The default seed is
# "MI355XCS"; the records are the LDS sweep's, with one checksum per phase in
# this order: the first six in the records of the first launch, xread in those
# of the second.
DEFAULT_CACHE_SWEEP_SEED = 0x4D493335_35584353
CACHE_SWEEP_PHASES = ("l1", "l2", "wt", "atomic", "scalar", "stream", "xread")
# nodeagent/nodeagent.h: NA_CACHE_PHASES of them, NA_CACHE_GRANULE,
# NA_CACHE_MAX_BYTES, NA_CACHE_TABLE_WORDS
CACHE_SWEEP_GRANULE = 4096  # slice_bytes is a multiple of this
CACHE_SWEEP_MAX_BYTES = 1 << 20
CACHE_SWEEP_TABLE_WORDS = 4096  # the scalar phase's read-only table
# the phases an XCD's L2 serves: failures of these on several CUs of one XCC
# point at that L2
CACHE_SWEEP_L2_PHASES = ("l2", "wt", "atomic", "stream", "xread")
# Floor of the default sweep's chip-wide stream rate: 0.70 x the 13950.1 GB/s
# median of five processes on MI355X (profiles/cache_sweep_mi355x.txt; 23
# bytes per clock and CU), the rule of the floors above. One workgroup per CU
# is latency-bound, so the figure is far under what the L2s deliver at full
# occupancy: a health floor, no benchmark. 0 disables the floor.
MIN_CACHE_SWEEP_GBS = 9765.1

# Chip-wide vector-unit sweep (nodeagent/valusweep.h). The default seed is
# "MI355XVS"; a record carries one checksum per phase, in this order. A listed
# wave's phase mask has two more bits: the record's own index and the
# placement of its workgroup.
DEFAULT_VALU_SWEEP_SEED = 0x4D493335_35585653
VALU_SWEEP_PHASES = ("rf", "rf_inv", "i32", "f32", "f64", "pk", "xlane", "trans", "stream")
VALU_SWEEP_MASK_NAMES = VALU_SWEEP_PHASES + ("index", "placement")
VALU_SWEEP_FIRST_VGPR = 32  # v0..v31 hold the test's own state and are not pattern-tested
# nodeagent/nodeagent.h: NA_VALU_MAX_ITERS (and NA_VALU_PHASES phases above)
VALU_SWEEP_MAX_ITERS = ((1 << 24) - 2048) // 2 - 1  # the stream phase is exact up to here
VALU_SWEEP_XLANE_MOVES = 8
NO_BAD_SLOT = (1 << 32) - 1
# FLOP per clock of one SIMD at the vector f32 peak (157.3 TFLOP/s over 1024
# SIMDs at 2.4 GHz): a ceiling, no floor
VALU_SWEEP_PEAK_FLOP_PER_CLK = 64
# Floor of the default sweep's chip-wide stream rate: 0.70 x the 108.72
# TFLOP/s median of five processes on MI355X
# (profiles/valu_sweep_mi355x.txt; 51.2 of the 64 FLOP per clock and SIMD).
# The device-to-device spread of VALU loops has not been measured; 0.70 is
# borrowed from the MFMA floor above. 0 disables the floor.
MIN_VALU_SWEEP_TFLOPS = 76.1

# Chip-wide load sweep (nodeagent/loadsweep.h): the matrix-core sweep's chain
# on four waves of every CU while the other four stream device memory through
# LDS. The default seed is "MI355XLD"; records and results are the
# matrix-core sweep's, one set per role.
DEFAULT_LOAD_SWEEP_SEED = 0x4D493335_35584C44
LOAD_SWEEP_ROLES = ("matrix", "stream")
# nodeagent/nodeagent.h: NA_LOAD_GRANULE, NA_LOAD_MAX_BYTES
LOAD_SWEEP_GRANULE = 16384  # slice_bytes is a multiple of this
LOAD_SWEEP_MAX_BYTES = 16 << 20
# Floors of the default sweep's two rates, reached together: 0.70 x the
# 1552.5 TFLOP/s and 3543.0 GB/s medians of five processes on MI355X
# (profiles/load_sweep_mi355x.txt; the chip held 1579 MHz under that load), the
# rule of the floors above and with the MFMA floor's caveat: integer operands
# held in registers, not comparable to GEMM benchmarks, and a memory stream of
# four latency-bound waves per CU, not the chip's copy bandwidth. The
# device-to-device spread under combined load has not been measured; 0.70 is
# borrowed from the MFMA floor. 0 disables a floor.
MIN_LOAD_SWEEP_TFLOPS = 1086.75
MIN_LOAD_SWEEP_GBS = 2480.1

# check()'s boolean self-tests in order: (method, GPUReport field, problem label)
_SELFTESTS = (
    ("fma_selftest", "fma_ok", "VALU FMA selftest"),
    ("mfma_selftest", "mfma_ok", "MFMA matrix-pipe selftest"),
    ("mfma_bf16_selftest", "mfma_bf16_ok", "MFMA bf16 selftest"),
    ("mfma_fp8_selftest", "mfma_fp8_ok", "MFMA fp8 selftest"),
    ("mfma_bf16_tile_check", None, "MFMA bf16 tile check"),
    ("mfma_fp8_tile_check", None, "MFMA fp8 tile check"),
    ("mfma_i8_tile_check", None, "MFMA i8 tile check"),
    ("mfma_f16_tile_check", None, "MFMA f16 tile check"),
    ("mfma_mx_tile_check", None, "MFMA MX-scaled tile check"),
    ("mfma_bf16_tile32_check", None, "MFMA 32x32 tile check"),
    ("lds_selftest", "lds_ok", "LDS selftest"),
)


class NodeAgentError(RuntimeError):
    pass


class MemtestAllocError(NodeAgentError):
    """The memtest region could not be allocated (busy GPU) — not a fault."""


def _shared_fields(cls, res) -> dict:
    """The fields that the C result ``res`` and the dataclass ``cls`` share by
    name, as keyword arguments for ``cls``; a converter adds the few that differ."""
    names = {f.name for f in fields(cls)}
    return {name: getattr(res, name) for name, _type in res._fields_ if name in names}


class _MemtestResultC(ctypes.Structure):
    _fields_ = [
        ("bytes_tested", ctypes.c_uint64),
        ("bad_words", ctypes.c_uint64),
        ("first_bad_offset", ctypes.c_uint64),
        ("xor_mask", ctypes.c_uint64),
    ]


@dataclass
class MemtestResult:
    """Outcome of a pattern verify. ``bad_words`` counts 64-bit words,
    ``first_bad_offset`` is a byte offset from the region start
    (``NO_BAD_OFFSET`` = none), ``xor_mask`` the OR of got^want over all bad
    words (the failing data bits)."""

    bytes_tested: int = 0
    bad_words: int = 0
    first_bad_offset: int = NO_BAD_OFFSET
    xor_mask: int = 0
    gbs: float = 0.0

    @property
    def ok(self) -> bool:
        return self.bad_words == 0

    def describe(self) -> str:
        return (
            f"{self.bad_words} bad 64-bit words in {self.bytes_tested} bytes, "
            f"first at offset {self.first_bad_offset:#x}, failing bits {self.xor_mask:#x}"
        )


class MfmaRecord(ctypes.Structure):
    """One wave of the matrix-core sweep (``na_mfma_record``): its checksum,
    the s_memtime / s_memrealtime deltas around its fold loop, its global
    wave index and the unit it ran on."""

    _fields_ = [
        ("checksum", ctypes.c_uint64),
        ("cycles", ctypes.c_uint64),
        ("realtime", ctypes.c_uint64),
        ("wave", ctypes.c_uint32),
        ("xcc", ctypes.c_uint32),
        ("se", ctypes.c_uint32),
        ("sh", ctypes.c_uint32),
        ("cu", ctypes.c_uint32),
        ("simd", ctypes.c_uint32),
    ]


class _MfmaSweepResultC(ctypes.Structure):
    _fields_ = [
        ("waves", ctypes.c_uint64),
        ("bad_waves", ctypes.c_uint64),
        ("units_seen", ctypes.c_uint64),
        ("bad_units", ctypes.c_uint64),
        ("first_bad_wave", ctypes.c_uint64),
        ("clock_mhz", ctypes.c_double),
        ("first_bad_unit", ctypes.c_uint32 * 5),
        ("listed", ctypes.c_uint32),
        ("bad_list", (ctypes.c_uint32 * 5) * MFMA_SWEEP_MAX_LISTED),
    ]


def mfma_unit_name(unit) -> str:
    """``(xcc, se, sh, cu[, simd])`` -> ``xcc2.se1.sh0.cu5[.simd3]``: the
    XCD, shader engine and shader array within it, CU within the array, and
    SIMD within the CU, as the hardware's XCC_ID / HW_ID registers number
    them."""
    name = "xcc{}.se{}.sh{}.cu{}".format(*unit[:4])
    return name + (f".simd{unit[4]}" if len(unit) > 4 else "")


@dataclass
class MfmaSweepResult:
    """Outcome of a sweep verify. A *unit* is a CU, ``(xcc, se, sh, cu)``;
    ``bad_simds`` lists the first distinct failing ``(xcc, se, sh, cu, simd)``
    (at most ``MFMA_SWEEP_MAX_LISTED``), the first being the unit of
    ``first_bad_wave``. ``tflops`` is 0 when only a verify was done."""

    dtype: str = "bf16"
    waves: int = 0
    bad_waves: int = 0
    units_seen: int = 0
    bad_units: int = 0
    first_bad_wave: int = NO_BAD_WAVE
    bad_simds: list = field(default_factory=list)
    clock_mhz: float = 0.0
    tflops: float = 0.0

    @property
    def ok(self) -> bool:
        return self.bad_waves == 0

    def describe(self) -> str:
        simds: dict = {}  # CU -> its failing SIMDs, in order of first failure
        for u in self.bad_simds:
            simds.setdefault(tuple(u[:4]), []).append(str(u[4]))
        names = ", ".join(f"{mfma_unit_name(cu)} simd {','.join(s)}" for cu, s in simds.items())
        more = ", ..." if len(self.bad_simds) == MFMA_SWEEP_MAX_LISTED else ""
        return (
            f"{self.bad_waves} of {self.waves} waves wrong on {self.bad_units} CU(s): "
            f"{names}{more}"
        )

    @classmethod
    def _from_c(cls, dtype: str, res: "_MfmaSweepResultC", tflops: float = 0.0):
        return cls(
            **_shared_fields(cls, res), dtype=dtype, tflops=tflops,
            bad_simds=[tuple(res.bad_list[i]) for i in range(res.listed)],
        )


class LoadSweepNoRoom(NodeAgentError):
    """The load sweep's region does not fit in free device memory (busy GPU) — not a fault."""


@dataclass
class LoadSweepResult:
    """Outcome of a load sweep verify: an ``MfmaSweepResult`` per role of
    ``LOAD_SWEEP_ROLES`` (the units of ``stream`` are those its waves ran on)
    and what the stream waves' own comparison saw, as a ``MemtestResult``
    whose offsets are relative to the region. ``tflops`` and ``gbs`` are the
    rates the two roles reached together, from the in-kernel clocks;
    ``matrix.clock_mhz`` is the clock under that load; ``overlap`` is the
    median over the workgroups of the shorter role's time over the longer's
    (0 when a role was off). All three are 0 when only a verify was done."""

    matrix: MfmaSweepResult = field(default_factory=MfmaSweepResult)
    stream: MfmaSweepResult = field(default_factory=MfmaSweepResult)
    mem: MemtestResult = field(default_factory=MemtestResult)
    tflops: float = 0.0
    gbs: float = 0.0
    overlap: float = 0.0

    @property
    def ok(self) -> bool:
        return self.matrix.ok and self.stream.ok and self.mem.ok

    def describe(self) -> str:
        """One sentence per failing role, then the in-kernel comparison."""
        parts = [
            f"{role} waves failed under combined load: {res.describe()}"
            for role, res in zip(LOAD_SWEEP_ROLES, (self.matrix, self.stream)) if not res.ok
        ]
        if not self.mem.ok:
            parts.append(f"stream comparison: {self.mem.describe()}")
        return "; ".join(parts)


class LdsRecord(ctypes.Structure):
    """One workgroup of the LDS sweep (``na_lds_record``): a checksum per
    phase of ``LDS_SWEEP_PHASES``, the in-kernel diagnosis (count of bad
    words, LDS byte offset of the first, OR of got^want, and the phase they
    were seen in), the s_memtime / s_memrealtime deltas around the stream
    phase, its index and the CU it ran on."""

    _fields_ = [
        ("checksum", ctypes.c_uint64 * len(LDS_SWEEP_PHASES)),
        ("bad_words", ctypes.c_uint64),
        ("first_bad_offset", ctypes.c_uint64),
        ("xor_mask", ctypes.c_uint64),
        ("cycles", ctypes.c_uint64),
        ("realtime", ctypes.c_uint64),
        ("workgroup", ctypes.c_uint32),
        ("bad_phase", ctypes.c_uint32),
        ("xcc", ctypes.c_uint32),
        ("se", ctypes.c_uint32),
        ("sh", ctypes.c_uint32),
        ("cu", ctypes.c_uint32),
    ]


class _LdsSweepResultC(ctypes.Structure):
    _fields_ = [
        ("workgroups", ctypes.c_uint64),
        ("bad_workgroups", ctypes.c_uint64),
        ("units_seen", ctypes.c_uint64),
        ("bad_units", ctypes.c_uint64),
        ("first_bad_workgroup", ctypes.c_uint64),
        ("bad_words", ctypes.c_uint64),
        ("first_bad_offset", ctypes.c_uint64),
        ("xor_mask", ctypes.c_uint64),
        ("clock_mhz", ctypes.c_double),
        ("median_bytes_per_clk", ctypes.c_double),
        ("min_bytes_per_clk", ctypes.c_double),
        ("max_bytes_per_clk", ctypes.c_double),
        ("first_bad_unit", ctypes.c_uint32 * 4),
        ("first_bad_phase", ctypes.c_uint32),
        ("listed", ctypes.c_uint32),
        ("bad_list", (ctypes.c_uint32 * 4) * LDS_SWEEP_MAX_LISTED),
    ]


@dataclass
class LdsSweepResult:
    """Outcome of an LDS sweep verify. A *unit* is a CU, ``(xcc, se, sh,
    cu)``; ``bad_cus`` lists the first distinct failing ones (at most
    ``LDS_SWEEP_MAX_LISTED``), the first being that of
    ``first_bad_workgroup``. ``first_bad_phase`` names the first failing phase
    of that workgroup ("index" when its record only sits in the wrong place);
    ``bad_words`` / ``first_bad_offset`` / ``xor_mask`` are the kernel's own
    diagnosis when that phase compares words (b32, b128, dma*). The rates are
    the stream phase's bytes per shader clock and CU over the workgroups;
    ``gbs`` is 0 when only a verify was done."""

    workgroups: int = 0
    bad_workgroups: int = 0
    units_seen: int = 0
    bad_units: int = 0
    first_bad_workgroup: int = NO_BAD_WORKGROUP
    first_bad_phase: str = ""
    bad_words: int = 0
    first_bad_offset: int = NO_BAD_OFFSET
    xor_mask: int = 0
    bad_cus: list = field(default_factory=list)
    clock_mhz: float = 0.0
    median_bytes_per_clk: float = 0.0
    min_bytes_per_clk: float = 0.0
    max_bytes_per_clk: float = 0.0
    gbs: float = 0.0

    @property
    def ok(self) -> bool:
        return self.bad_workgroups == 0

    def describe(self) -> str:
        names = ", ".join(mfma_unit_name(u) for u in self.bad_cus)
        more = ", ..." if len(self.bad_cus) == LDS_SWEEP_MAX_LISTED else ""
        where = ""
        if self.first_bad_offset != NO_BAD_OFFSET:
            where = (
                f", {self.bad_words} bad words, first at LDS offset {self.first_bad_offset:#x} "
                f"(bank {self.first_bad_offset // 4 % 64}), failing bits {self.xor_mask:#010x}"
            )
        return (
            f"{self.bad_workgroups} of {self.workgroups} workgroups wrong on {self.bad_units} "
            f"CU(s): {names}{more}; first in phase {self.first_bad_phase}{where}"
        )

    @classmethod
    def _from_c(cls, res: "_LdsSweepResultC", gbs: float = 0.0):
        phase = ""
        if res.first_bad_workgroup != NO_BAD_WORKGROUP:
            phase = (LDS_SWEEP_PHASES + ("index",))[min(res.first_bad_phase, len(LDS_SWEEP_PHASES))]
        # first_bad_phase is a code in C and a name here
        return cls(**{
            **_shared_fields(cls, res), "first_bad_phase": phase, "gbs": gbs,
            "bad_cus": [tuple(res.bad_list[i]) for i in range(res.listed)],
        })


@dataclass
class CacheSweepResult(LdsSweepResult):
    """Outcome of a cache sweep verify: the LDS sweep's shape.
    ``first_bad_phase`` is one of ``CACHE_SWEEP_PHASES`` or "index",
    ``first_bad_offset`` the byte offset within the workgroup's slice, and
    the diagnosis triple is filled when that phase compares words in the
    kernel (l1, l2, wt, atomic, xread). The rates are the stream phase's bytes
    per shader clock and CU, read from the L2."""

    def describe(self) -> str:
        names = ", ".join(mfma_unit_name(u) for u in self.bad_cus)
        more = ", ..." if len(self.bad_cus) == LDS_SWEEP_MAX_LISTED else ""
        if (self.first_bad_phase in CACHE_SWEEP_L2_PHASES and len(self.bad_cus) >= 2
                and len({u[0] for u in self.bad_cus}) == 1 and self.bad_units == len(self.bad_cus)):
            names, more = f"all on xcc{self.bad_cus[0][0]}: suspect its L2", ""
        where = ""
        if self.first_bad_offset != NO_BAD_OFFSET:
            where = (
                f", {self.bad_words} bad words, first at slice offset {self.first_bad_offset:#x}, "
                f"failing bits {self.xor_mask:#010x}"
            )
        return (
            f"{self.bad_workgroups} of {self.workgroups} workgroups wrong on {self.bad_units} "
            f"CU(s): {names}{more}; first in phase {self.first_bad_phase}{where}"
        )

    @classmethod
    def _from_c(cls, res: "_LdsSweepResultC", gbs: float = 0.0):
        out = super()._from_c(res, gbs)
        if res.first_bad_workgroup != NO_BAD_WORKGROUP:
            out.first_bad_phase = (CACHE_SWEEP_PHASES + ("index",))[
                min(res.first_bad_phase, len(CACHE_SWEEP_PHASES))]
        return out


class ValuRecord(ctypes.Structure):
    """One wave of the vector-unit sweep (``na_valu_record``): a checksum per
    phase of ``VALU_SWEEP_PHASES``, the s_memtime / s_memrealtime deltas around
    the stream phase, its global wave index, the unit it ran on, and the
    kernel's own diagnosis of the register-file phases (count of wrong
    registers, slot and lane of the first, OR of got^want)."""

    _fields_ = [
        ("checksum", ctypes.c_uint64 * len(VALU_SWEEP_PHASES)),
        ("cycles", ctypes.c_uint64),
        ("realtime", ctypes.c_uint64),
        ("wave", ctypes.c_uint32),
        ("xcc", ctypes.c_uint32),
        ("se", ctypes.c_uint32),
        ("sh", ctypes.c_uint32),
        ("cu", ctypes.c_uint32),
        ("simd", ctypes.c_uint32),
        ("rf_bad", ctypes.c_uint32),
        ("rf_first_slot", ctypes.c_uint32),
        ("rf_first_lane", ctypes.c_uint32),
        ("rf_xor", ctypes.c_uint32),
    ]


class _ValuSweepResultC(ctypes.Structure):
    _fields_ = [
        ("waves", ctypes.c_uint64),
        ("bad_waves", ctypes.c_uint64),
        ("cus_seen", ctypes.c_uint64),
        ("simds_seen", ctypes.c_uint64),
        ("trans_unchecked", ctypes.c_uint64),
        ("trans_consensus", ctypes.c_uint64),
        ("median_cycles", ctypes.c_uint64),
        ("clock_mhz", ctypes.c_double),
        ("median_flop_per_clk", ctypes.c_double),
        ("min_flop_per_clk", ctypes.c_double),
        ("tflops", ctypes.c_double),
        ("rf_bad", ctypes.c_uint32),
        ("rf_first_slot", ctypes.c_uint32),
        ("rf_first_lane", ctypes.c_uint32),
        ("rf_xor", ctypes.c_uint32),
        ("listed", ctypes.c_uint32),
        ("bad_list", (ctypes.c_uint32 * 7) * VALU_SWEEP_MAX_LISTED),
    ]


def valu_slot_name(slot: int) -> str:
    """Register of register-file slot ``slot``: ``a0..a255``, then
    ``v32..v255``; slots from 512 are the same registers in the inverted
    phase."""
    slot &= 511
    return f"a{slot}" if slot < 256 else f"v{slot - 256 + VALU_SWEEP_FIRST_VGPR}"


@dataclass
class ValuSweepResult:
    """Outcome of a vector-unit sweep verify. ``bad`` lists the first bad
    waves (at most ``VALU_SWEEP_MAX_LISTED``) as ``(wave, (xcc, se, sh, cu,
    simd), [names of the phases that failed])``; ``bad_waves`` is the full
    count. ``trans_unchecked`` says the transcendental phase, which is checked
    by consensus among the records, had fewer than 3 records or no strict
    majority: not a failure. The ``rf_*`` fields are the kernel's own
    diagnosis of the first bad wave when it failed a register-file phase.
    The rates are the stream phase's FLOP per shader clock and SIMD;
    ``tflops`` comes from the in-kernel stamps, never from launch time."""

    waves: int = 0
    bad_waves: int = 0
    cus_seen: int = 0
    simds_seen: int = 0
    trans_unchecked: bool = True
    trans_consensus: int = 0
    median_cycles: int = 0
    clock_mhz: float = 0.0
    median_flop_per_clk: float = 0.0
    min_flop_per_clk: float = 0.0
    tflops: float = 0.0
    rf_bad: int = 0
    rf_first_slot: int = NO_BAD_SLOT
    rf_first_lane: int = NO_BAD_SLOT
    rf_xor: int = 0
    bad: list = field(default_factory=list)

    @property
    def ok(self) -> bool:
        return self.bad_waves == 0

    def describe(self) -> str:
        names = ", ".join(
            f"{mfma_unit_name(unit)} ({','.join(phases)})" for _wave, unit, phases in self.bad
        )
        more = ", ..." if self.bad_waves > len(self.bad) else ""
        where = ""
        if self.rf_bad:
            where = (
                f"; first: {self.rf_bad} wrong registers, first {valu_slot_name(self.rf_first_slot)}"
                f"{' inverted' if self.rf_first_slot >= 512 else ''} lane {self.rf_first_lane}, "
                f"failing bits {self.rf_xor:#010x}"
            )
        return f"{self.bad_waves} of {self.waves} waves wrong: {names}{more}{where}"

    @classmethod
    def _from_c(cls, res: "_ValuSweepResultC"):
        bad = []
        for i in range(res.listed):
            row = list(res.bad_list[i])
            phases = [n for p, n in enumerate(VALU_SWEEP_MASK_NAMES) if row[6] >> p & 1]
            bad.append((row[0], tuple(row[1:6]), phases))
        return cls(**{
            **_shared_fields(cls, res), "trans_unchecked": bool(res.trans_unchecked), "bad": bad,
        })


# The binding of nodeagent/nodeagent.h: one row per prototype, in its order,
# as symbol -> (restype, argtypes) with the types spelled as the prototype
# spells them. _load_lib applies it, so a plain Python int reaches a 64-bit
# or pointer parameter whole. tests/test_nodeagent_abi.py holds the table and
# the Structure classes above against the header.
_int, _i64, _u64, _void_p = ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_void_p
_P = ctypes.POINTER
_int_p, _i64_p, _u64_p, _double_p = _P(_int), _P(_i64), _P(ctypes.c_uint64), _P(ctypes.c_double)
_char_p = _P(ctypes.c_char)  # a buffer the callee fills
_DEV = (_int, (_int,))  # int fn(int dev)
_BANDWIDTH = (_int, (_int, _i64, _int, _double_p))
_CHECK_RUN = (_int, (_int, _int, _void_p, _int))
_CHECK_VERIFY = (_int, (_int, _void_p, _int))
_WAVE_EXPECTED = (_int, (_u64, _u64, _int, _u64_p))
_MATRIX_RUN = (_int, (_int, _int, _int, _int, _u64, _P(MfmaRecord), _i64, _double_p))
_MATRIX_VERIFY = (_int, (_P(MfmaRecord), _i64, _int, _u64, _P(_MfmaSweepResultC)))
_MATRIX_SWEEP = (_int, (_int, _int, _int, _int, _u64, _P(_MfmaSweepResultC), _double_p))
_ABI = {
    "na_last_error": (ctypes.c_char_p, ()),
    "na_device_count": (_int, (_int_p,)),
    "na_device_info": (_int, (_int, _char_p, _int, _char_p, _int, _i64_p, _int_p, _int_p)),
    "na_hbm_bandwidth": _BANDWIDTH,
    "na_copy_run": (_int, (_int, _void_p, _void_p, _i64, _int, _int)),
    "na_fma_selftest": _DEV,
    "na_mfma_check_run": _CHECK_RUN,
    "na_mfma_check_verify": _CHECK_VERIFY,
    "na_mfma_selftest": _DEV,
    "na_mfma_bf16_selftest": _DEV,
    "na_mfma_fp8_selftest": _DEV,
    "na_mfma_bf16_tile_check": _DEV,
    "na_mfma_f16_tile_check": _DEV,
    "na_mfma_fp8_tile_check": _DEV,
    "na_mfma_i8_tile_check": _DEV,
    "na_mfma_bf16_tile32_check": _DEV,
    "na_mfma_mx_tile_check": _DEV,
    "na_mx_decode": (_int, (_int, _int, _P(ctypes.c_float))),
    "na_mx_pack": (_int, (_int, _int_p, _int, _P(ctypes.c_uint32), _int)),
    "na_mx_check_run": _CHECK_RUN,
    "na_mx_check_verify": _CHECK_VERIFY,
    "na_mx_checks": _DEV,
    "na_lds_selftest": (_int, (_int, _i64_p)),
    "na_sdma_bandwidth": _BANDWIDTH,
    "na_p2p_matrix": (_int, (_int, _int_p)),
    "na_p2p_bandwidth": (_int, (_int, _int, _i64, _int, _double_p)),
    "na_mem_info": (_int, (_int, _i64_p, _i64_p)),
    "na_memtest_fill": (_int, (_int, _void_p, _i64, _u64, _int)),
    "na_memtest_verify": (_int, (_int, _void_p, _i64, _u64, _int, _int, _P(_MemtestResultC))),
    "na_hbm_memtest_passes": (
        _int, (_int, _i64, _int, _u64, _P(_MemtestResultC), _double_p, _double_p)),
    "na_hbm_memtest": (_int, (_int, _i64, _int, _u64, _P(_MemtestResultC), _double_p)),
    "na_mfma_sweep_expected": _WAVE_EXPECTED,
    "na_mfma_sweep_run": _MATRIX_RUN,
    "na_mfma_sweep_verify": _MATRIX_VERIFY,
    "na_mfma_sweep": _MATRIX_SWEEP,
    "na_mx_sweep_expected": _WAVE_EXPECTED,
    "na_mx_sweep_run": _MATRIX_RUN,
    "na_mx_sweep_verify": _MATRIX_VERIFY,
    "na_mx_sweep": _MATRIX_SWEEP,
    "na_lds_sweep_allocation": (_int, (_int, _i64_p)),
    "na_lds_sweep_expected": (_int, (_u64, _u64, _i64, _int, _u64_p, _int)),
    "na_lds_sweep_run": (_int, (_int, _int, _i64, _int, _u64, _P(LdsRecord), _i64, _double_p)),
    "na_lds_sweep_verify": (_int, (_P(LdsRecord), _i64, _i64, _int, _u64, _P(_LdsSweepResultC))),
    "na_lds_sweep": (_int, (_int, _int, _i64, _int, _u64, _P(_LdsSweepResultC), _double_p)),
    "na_cache_sweep_expected": (_int, (_u64, _u64, _u64, _i64, _int, _u64_p, _int)),
    "na_cache_sweep_run": (_int, (_int, _int, _i64, _int, _u64, _P(LdsRecord), _i64, _double_p)),
    "na_cache_sweep_verify": (
        _int, (_P(LdsRecord), _i64, _i64, _int, _u64, _P(_LdsSweepResultC))),
    "na_cache_sweep": (_int, (_int, _int, _i64, _int, _u64, _P(_LdsSweepResultC), _double_p)),
    "na_valu_sweep_xlane_table": (_int, (_int, _int_p, _int)),
    "na_valu_sweep_slots": (_int, ()),
    "na_valu_sweep_expected": _WAVE_EXPECTED,
    "na_valu_sweep_run": (_int, (_int, _int, _int, _u64, _P(ValuRecord), _i64, _double_p)),
    "na_valu_sweep_verify": (_int, (_P(ValuRecord), _i64, _int, _u64, _P(_ValuSweepResultC))),
    "na_valu_sweep": (_int, (_int, _int, _int, _u64, _P(_ValuSweepResultC))),
    "na_load_sweep_stream_expected": (_int, (_u64, _u64, _i64, _int, _u64_p, _int)),
    "na_load_sweep_run": (
        _int, (_int, _int, _int, _int, _void_p, _i64, _int, _u64, _P(MfmaRecord), _P(MfmaRecord),
               _i64, _P(_MemtestResultC), _double_p)),
    "na_load_sweep_verify": (
        _int, (_P(MfmaRecord), _P(MfmaRecord), _i64, _int, _i64, _int, _u64,
               _P(_MfmaSweepResultC), _P(_MfmaSweepResultC))),
    "na_load_sweep": (
        _int, (_int, _int, _int, _int, _i64, _int, _u64, _P(_MfmaSweepResultC),
               _P(_MfmaSweepResultC), _P(_MemtestResultC), _double_p, _double_p, _double_p)),
}


def _load_lib() -> ctypes.CDLL:
    for p in _SEARCH_PATHS:
        if os.path.exists(p):
            lib = ctypes.CDLL(os.path.abspath(p))
            for symbol, (restype, argtypes) in _ABI.items():
                try:
                    fn = getattr(lib, symbol)
                except AttributeError:
                    raise NodeAgentError(f"{p} does not export {symbol}; rebuild it") from None
                fn.restype, fn.argtypes = restype, argtypes
            return lib
    raise NodeAgentError(
        f"{_LIB_NAME} not found (searched {', '.join(_SEARCH_PATHS)}); "
        "build it with __graft_entry__.build() / make -C nodeagent"
    )


@dataclass
class GPUReport:
    index: int
    name: str = ""
    arch: str = ""
    hbm_gb: float = 0.0
    cus: int = 0
    hbm_bw_gbs: float = 0.0
    fma_ok: bool = False
    mfma_ok: bool = False
    mfma_bf16_ok: bool = False
    mfma_fp8_ok: bool = False
    lds_ok: bool = False
    lds_bytes_tested: int = 0
    # chip-wide LDS sweep (opt-in; all "not run" by default)
    lds_sweep_gbs: float = 0.0
    lds_sweep_min_cu_bytes_per_clk: float = 0.0
    lds_sweep_units_seen: int = 0
    lds_sweep_bad_workgroups: int = 0
    # chip-wide cache sweep (opt-in; all "not run" by default)
    cache_sweep_gbs: float = 0.0
    cache_sweep_min_cu_bytes_per_clk: float = 0.0
    cache_sweep_units_seen: int = 0
    cache_sweep_bad_workgroups: int = 0
    # chip-wide vector-unit sweep (opt-in; all "not run" by default)
    valu_sweep_tflops: float = 0.0
    valu_sweep_min_simd_flop_per_clk: float = 0.0
    valu_sweep_simds_seen: int = 0
    valu_sweep_bad_waves: int = 0
    valu_sweep_trans_unchecked: bool = False
    # chip-wide load sweep (opt-in; all "not run" by default)
    load_sweep_tflops: float = 0.0
    load_sweep_gbs: float = 0.0
    load_sweep_clock_mhz: float = 0.0  # under combined load; informational, no floor
    load_sweep_overlap: float = 0.0
    load_sweep_units_seen: int = 0
    load_sweep_bad_waves: int = 0  # of both roles
    load_sweep_bad_words: int = 0
    load_sweep_skipped: str = ""  # reason, when requested but not run
    sdma_bw_gbs: float = 0.0
    healthy: bool = False
    problems: list = field(default_factory=list)
    # HBM data-integrity test (opt-in; all "not run" by default)
    hbm_memtest_bytes: int = 0
    hbm_memtest_bad_words: int = 0
    hbm_memtest_gbs: float = 0.0
    hbm_memtest_skipped: str = ""  # reason, when requested but not run
    # chip-wide matrix-core sweep (opt-in; all "not run" by default)
    mfma_sweep_tflops: float = 0.0
    mfma_sweep_fp8_tflops: float = 0.0
    mfma_sweep_clock_mhz: float = 0.0  # bf16 run; informational, no floor
    mfma_sweep_units_seen: int = 0
    mfma_sweep_bad_waves: int = 0
    # single-wave MX checks and chip-wide MX sweep (opt-in; "not run" by default)
    mx_checks_run: int = 0  # kinds run
    mx_checks_failed: list = field(default_factory=list)  # names of the kinds that failed
    mx_sweep_fp4_tflops: float = 0.0
    mx_sweep_fp6_tflops: float = 0.0
    mx_sweep_bad_waves: int = 0


@dataclass
class NodeReport:
    healthy: bool = False
    gpu_count: int = 0
    gpus: list = field(default_factory=list)
    xgmi_p2p: list = field(default_factory=list)
    xgmi_bw_gbs: list = field(default_factory=list)
    problems: list = field(default_factory=list)


class NodeAgent:
    def __init__(self):
        self.lib = _load_lib()

    def _err(self) -> str:
        return (self.lib.na_last_error() or b"").decode()

    def _check(self, rc: int, what: str, ok=(NA_OK,)) -> None:
        """Raise ``NodeAgentError`` with ``what`` and ``na_last_error`` unless
        the C code ``rc`` is one of ``ok``."""
        if rc not in ok:
            raise NodeAgentError(f"{what}: {self._err()}")

    def device_count(self) -> int:
        n = ctypes.c_int(0)
        self._check(self.lib.na_device_count(ctypes.byref(n)), "device_count")
        return n.value

    def device_info(self, dev: int) -> tuple:
        name = ctypes.create_string_buffer(256)
        arch = ctypes.create_string_buffer(256)
        hbm = ctypes.c_longlong(0)
        cus = ctypes.c_int(0)
        clk = ctypes.c_int(0)
        rc = self.lib.na_device_info(
            dev, name, 256, arch, 256, ctypes.byref(hbm), ctypes.byref(cus), ctypes.byref(clk)
        )
        self._check(rc, f"device_info({dev})")
        return name.value.decode(), arch.value.decode(), hbm.value, cus.value

    def hbm_bandwidth(self, dev: int, bytes_: int = 1 << 30, iters: int = 10) -> float:
        out = ctypes.c_double(0)
        rc = self.lib.na_hbm_bandwidth(dev, bytes_, iters, ctypes.byref(out))
        self._check(rc, f"hbm_bandwidth({dev})")
        return out.value

    def copy_run(self, dev: int, src: int, dst: int, bytes_: int, workgroups: int = 0,
                 threads: int = 0) -> int:
        """One synchronised launch of the bandwidth probe's copy kernel on
        caller-owned device memory (``src`` and ``dst`` 16-byte aligned and
        disjoint, ``bytes_`` a positive multiple of 16, ``workgroups`` up to
        65535, ``threads`` a multiple of 64 up to 1024; 0 for either is the
        probe's own 16384 x 1024). Returns the C return code (``NA_ERR_ARG``
        for anything outside that range)."""
        return self.lib.na_copy_run(dev, src, dst, bytes_, workgroups, threads)

    def fma_selftest(self, dev: int) -> bool:
        return self.lib.na_fma_selftest(dev) == 0

    def mfma_selftest(self, dev: int) -> bool:
        return self.lib.na_mfma_selftest(dev) == 0

    def mfma_bf16_selftest(self, dev: int) -> bool:
        """v_mfma_f32_16x16x32_bf16 — the CDNA4 training datapath."""
        return self.lib.na_mfma_bf16_selftest(dev) == 0

    def mfma_fp8_selftest(self, dev: int) -> bool:
        """v_mfma_f32_16x16x32_fp8_fp8 (E4M3) — the serving datapath."""
        return self.lib.na_mfma_fp8_selftest(dev) == 0

    def mfma_bf16_tile_check(self, dev: int) -> bool:
        """Layout-correct 16x16x32 bf16 GEMM tile with asymmetric data vs
        an exact host reference — catches fragment-mapping errors the
        uniform-operand self-tests cannot."""
        return self.lib.na_mfma_bf16_tile_check(dev) == 0

    def mfma_fp8_tile_check(self, dev: int) -> bool:
        """E4M3 variant of the layout-correct tile check."""
        return self.lib.na_mfma_fp8_tile_check(dev) == 0

    def mfma_i8_tile_check(self, dev: int) -> bool:
        """int8 K=64 variant (v_mfma_i32_16x16x64_i8) of the tile check."""
        return self.lib.na_mfma_i8_tile_check(dev) == 0

    def mfma_f16_tile_check(self, dev: int) -> bool:
        """f16 variant (v_mfma_f32_16x16x32_f16) of the tile check."""
        return self.lib.na_mfma_f16_tile_check(dev) == 0

    def mfma_bf16_tile32_check(self, dev: int) -> bool:
        """32x32x16 bf16 tile — the other CDNA4 tile geometry, with its
        distinct C/D fragment map."""
        return self.lib.na_mfma_bf16_tile32_check(dev) == 0

    def mfma_mx_tile_check(self, dev: int) -> bool:
        """Block-scaled MX path (v_mfma_scale_f32_16x16x128_f8f6f4) on E4M3
        operands only, with one scale for all of A (1.0, then 2.0) and B's
        at 1.0, vs exact host references. The other operand formats (fp4,
        fp6, bf6, bf8), per-lane scales and the scale byte select are
        covered by ``mx_checks``."""
        return self.lib.na_mfma_mx_tile_check(dev) == 0

    def mfma_check_run(self, dev: int, kind: str):
        """Launch the one wave of check ``kind`` (a key of ``MFMA_CHECK_KINDS``)
        and return its raw words as a ctypes array of 1024 uint32, of which
        the kind's first 256 (all 1024 for ``bf16_tile32``) are written."""
        return self._check_run("mfma", MFMA_CHECK_KINDS, dev, kind)

    def mfma_check_verify(self, kind: str, words) -> int:
        """Compare a kind's words with the exact host reference (needs no GPU).
        Returns the C code; on ``NA_ERR_VERIFY`` ``na_last_error`` names the word."""
        return self._check_verify("mfma", MFMA_CHECK_KINDS, kind, words)

    # The single-wave checks' two families, "mfma" and "mx", differ in symbol
    # prefix and kind table.

    def _check_run(self, fam: str, kinds: dict, dev: int, kind: str):
        words = (ctypes.c_uint32 * MFMA_CHECK_MAX_WORDS)()
        rc = getattr(self.lib, f"na_{fam}_check_run")(dev, kinds[kind], words, len(words))
        self._check(rc, f"{fam}_check_run({dev}, {kind})")
        return words

    def _check_verify(self, fam: str, kinds: dict, kind: str, words) -> int:
        return getattr(self.lib, f"na_{fam}_check_verify")(kinds[kind], words, len(words))

    # -- single-wave MX checks ------------------------------------------------

    def mx_decode(self, fmt: str, code: int) -> float:
        """Value of ``code`` in format ``fmt`` (a key of ``MX_FORMATS``), by
        the decoder the host references use (needs no GPU)."""
        out = ctypes.c_float(0)
        rc = self.lib.na_mx_decode(MX_FORMATS[fmt], code, ctypes.byref(out))
        self._check(rc, f"mx_decode({fmt}, {code})")
        return out.value

    def mx_pack(self, fmt: str, codes) -> list:
        """``codes`` (a multiple of 32 of them) packed the way the kernels
        pack a lane's fragments: element i of a fragment at bit i * width,
        little-endian across 32-bit words (needs no GPU)."""
        n = len(codes)
        words = (ctypes.c_uint32 * max(n * MX_FORMAT_BITS[fmt] // 32, 1))()
        rc = self.lib.na_mx_pack(MX_FORMATS[fmt], (ctypes.c_int * max(n, 1))(*codes), n, words,
                                 len(words))
        self._check(rc, f"mx_pack({fmt})")
        return list(words)

    def mx_check_run(self, dev: int, kind: str):
        """Launch the one wave of MX check ``kind`` (a key of
        ``MX_CHECK_KINDS``) and return its raw words as a ctypes array of
        1024 uint32, of which the kind's first 256 (all 1024 for ``fp4_32``)
        are written: float32 bit patterns."""
        return self._check_run("mx", MX_CHECK_KINDS, dev, kind)

    def mx_check_verify(self, kind: str, words) -> int:
        """Compare a kind's words with the exact host reference (needs no GPU).
        Returns the C code; on ``NA_ERR_VERIFY`` ``na_last_error`` names the word."""
        return self._check_verify("mx", MX_CHECK_KINDS, kind, words)

    def mx_checks(self, dev: int) -> bool:
        """Every kind of ``MX_CHECK_KINDS`` in turn, one wave each, stopping at
        the first that fails (``na_last_error`` names its first wrong word)."""
        return self.lib.na_mx_checks(dev) == NA_OK

    def _run_mx_checks(self, g: GPUReport) -> None:
        for kind in MX_CHECK_KINDS:  # all of them: each failure names its own word
            words = self.mx_check_run(g.index, kind)
            g.mx_checks_run += 1
            if self.mx_check_verify(kind, words) != NA_OK:
                g.mx_checks_failed.append(kind)
                g.problems.append(f"MX check {kind} failed: {self._err()}")

    def lds_selftest(self, dev: int) -> tuple:
        """(ok, bytes_tested): whole-LDS pattern write/swizzled-read check."""
        tested = ctypes.c_longlong(0)
        rc = self.lib.na_lds_selftest(dev, ctypes.byref(tested))
        return rc == 0, tested.value

    def sdma_bandwidth(self, dev: int, bytes_: int = 512 << 20, iters: int = 10) -> float:
        """D2D copy through the SDMA engines — RCCL's xGMI transport hardware."""
        out = ctypes.c_double(0)
        rc = self.lib.na_sdma_bandwidth(dev, bytes_, iters, ctypes.byref(out))
        self._check(rc, f"sdma_bandwidth({dev})")
        return out.value

    # -- HBM data integrity --------------------------------------------------

    def mem_info(self, dev: int) -> tuple:
        """(free_bytes, total_bytes) of device memory right now."""
        free = ctypes.c_longlong(0)
        total = ctypes.c_longlong(0)
        rc = self.lib.na_mem_info(dev, ctypes.byref(free), ctypes.byref(total))
        self._check(rc, f"mem_info({dev})")
        return free.value, total.value

    def memtest_fill(self, dev: int, ptr: int, bytes_: int,
                     seed: int = DEFAULT_MEMTEST_SEED, invert: bool = False) -> int:
        """Write the test pattern to caller-owned device memory (``ptr``
        16-byte aligned, ``bytes_`` a positive multiple of 16). Returns the
        C return code (``NA_ERR_ARG`` for a bad pointer/size)."""
        return self.lib.na_memtest_fill(dev, ptr, bytes_, seed, int(bool(invert)))

    def memtest_verify(self, dev: int, ptr: int, bytes_: int,
                       seed: int = DEFAULT_MEMTEST_SEED, invert: bool = False,
                       flip: bool = False) -> tuple:
        """Compare caller-owned device memory against the pattern; with
        ``flip`` also store the complement of the EXPECTED pattern. Returns
        ``(rc, MemtestResult)``; rc is ``NA_ERR_VERIFY`` on any mismatch."""
        res = _MemtestResultC()
        rc = self.lib.na_memtest_verify(
            dev, ptr, bytes_, seed, int(bool(invert)), int(bool(flip)), ctypes.byref(res),
        )
        if rc not in (NA_OK, NA_ERR_VERIFY):
            return rc, MemtestResult()
        return rc, MemtestResult(**_shared_fields(MemtestResult, res))

    def hbm_memtest(self, dev: int, bytes_: int, rounds: int = 1,
                    seed: int = DEFAULT_MEMTEST_SEED) -> MemtestResult:
        """Pattern-test ``bytes_`` of HBM the agent allocates itself (in
        chunks): per round fill(seed+r) -> verify+invert -> verify, so every
        cell is read back at both polarities; the pattern is a bijection of
        the address, so aliased address lines mismatch too. Mismatches come
        back in the result (``.ok`` False), not as an exception.

        Any size from 16 bytes is allowed, but a region under 512 MiB is
        served largely from the 256 MiB Infinity Cache rather than DRAM —
        it still checks the data path, not the HBM cells. ECC-corrected
        single-bit errors are invisible to this test by design."""
        res = _MemtestResultC()
        gbs = ctypes.c_double(0)
        rc = self.lib.na_hbm_memtest(
            dev, bytes_, rounds, seed, ctypes.byref(res), ctypes.byref(gbs)
        )
        if rc not in (NA_OK, NA_ERR_VERIFY):
            err = self._err()
            cls = MemtestAllocError if "allocation failed" in err else NodeAgentError
            raise cls(f"hbm_memtest({dev}): {err}")
        return MemtestResult(**_shared_fields(MemtestResult, res), gbs=gbs.value)

    def _run_memtest(self, g: GPUReport, memtest_bytes: int) -> None:
        free, _total = self.mem_info(g.index)
        want = min(memtest_bytes, free * MEMTEST_FREE_FRACTION_PCT // 100) & ~15
        if want < 16:
            g.hbm_memtest_skipped = (
                f"only {free} bytes of device memory free; nothing left to test"
            )
            return
        try:
            res = self.hbm_memtest(g.index, want)
        except MemtestAllocError as e:
            # a busy GPU must not get its node replaced for lack of free memory
            g.hbm_memtest_skipped = str(e)
            return
        g.hbm_memtest_bytes = res.bytes_tested
        g.hbm_memtest_bad_words = res.bad_words
        g.hbm_memtest_gbs = round(res.gbs, 1)
        if not res.ok:
            g.problems.append(f"HBM memtest: {res.describe()}")

    # -- what the chip-wide sweeps' wrappers share ------------------------------
    #
    # The whole-sweep entry points (na_*_sweep) are the ones check() reaches,
    # so the tests' stand-in libraries define them, and those read the seed
    # and lds_bytes through ``.value``. _matrix_sweep, lds_sweep, cache_sweep and
    # valu_sweep therefore still hand them over in their C types; the binding accepts
    # either form. Every other call passes plain ints.

    def _sweep_run(self, what, record_type, n, *args) -> tuple:
        """``na_<what>`` with ``args`` ahead of the ``n`` records it fills.
        Returns ``(records, ms)``."""
        recs = (record_type * max(n, 1))()
        ms = ctypes.c_double(0)
        dev = args[0]
        rc = getattr(self.lib, f"na_{what}")(*args, recs, n, ctypes.byref(ms))
        self._check(rc, f"{what}({dev})")
        return recs, ms.value

    def _sweep_verify(self, what, recs, args, res, wrap, empty) -> tuple:
        """``na_<what>`` on ``recs`` with ``args`` between the record count and
        the C result ``res``. Returns ``(rc, wrap(res))``, or ``(rc, empty())``
        when the call itself was refused."""
        rc = getattr(self.lib, f"na_{what}")(recs, len(recs), *args, ctypes.byref(res))
        return rc, wrap(res) if rc in (NA_OK, NA_ERR_VERIFY) else empty()

    # The matrix-core sweep's two families, "mfma" (dtypes) and "mx" (formats),
    # differ in symbol prefix, code table and the word for a code.

    @staticmethod
    def _matrix_code(fam: str, name: str) -> int:
        codes, word = ((MFMA_SWEEP_DTYPES, "dtype") if fam == "mfma"
                       else (MX_SWEEP_FORMATS, "format"))
        if name not in codes:
            raise NodeAgentError(f"{fam} sweep: {word} {name!r} is not one of {', '.join(codes)}")
        return codes[name]

    def _matrix_sweep_expected(self, fam, wave, outer, seed) -> int:
        out = ctypes.c_uint64(0)
        rc = getattr(self.lib, f"na_{fam}_sweep_expected")(seed, wave, outer, ctypes.byref(out))
        self._check(rc, f"{fam}_sweep_expected")
        return out.value

    def _matrix_sweep_run(self, fam, dev, name, workgroups, outer, seed) -> tuple:
        return self._sweep_run(
            f"{fam}_sweep_run", MfmaRecord, max(workgroups, 0) * MFMA_SWEEP_WAVES_PER_WG,
            dev, self._matrix_code(fam, name), workgroups, outer, seed,
        )

    def _matrix_sweep_verify(self, fam, recs, outer, seed, name) -> tuple:
        return self._sweep_verify(
            f"{fam}_sweep_verify", recs, (outer, seed), _MfmaSweepResultC(),
            lambda res: MfmaSweepResult._from_c(name, res), lambda: MfmaSweepResult(name),
        )

    def _matrix_sweep(self, fam, dev, name, workgroups, outer, seed) -> MfmaSweepResult:
        res = _MfmaSweepResultC()
        tflops = ctypes.c_double(0)
        rc = getattr(self.lib, f"na_{fam}_sweep")(
            dev, self._matrix_code(fam, name), workgroups, outer, ctypes.c_ulonglong(seed),
            ctypes.byref(res), ctypes.byref(tflops),
        )
        self._check(rc, f"{fam}_sweep({dev}, {name})", (NA_OK, NA_ERR_VERIFY))
        return MfmaSweepResult._from_c(name, res, tflops.value)

    # -- chip-wide matrix-core sweep ------------------------------------------

    def mfma_sweep_expected(self, wave: int, outer: int,
                            seed: int = DEFAULT_MFMA_SWEEP_SEED) -> int:
        """Checksum wave ``wave`` must report after ``outer`` folds (host
        arithmetic only; needs no GPU)."""
        return self._matrix_sweep_expected("mfma", wave, outer, seed)

    def mfma_sweep_run(self, dev: int, dtype: str = "bf16", workgroups: int = 1,
                       outer: int = 1, seed: int = DEFAULT_MFMA_SWEEP_SEED) -> tuple:
        """One launch of ``workgroups`` x 4 waves, each through ``outer``
        folds of 64 MFMAs. Returns ``(records, ms)``: a ctypes array of
        ``MfmaRecord`` (record i is wave i) and the HIP-event time."""
        return self._matrix_sweep_run("mfma", dev, dtype, workgroups, outer, seed)

    def mfma_sweep_verify(self, recs, outer: int, seed: int = DEFAULT_MFMA_SWEEP_SEED,
                          dtype: str = "bf16") -> tuple:
        """Compare every record against the host reference. Returns
        ``(rc, MfmaSweepResult)``; rc is ``NA_ERR_VERIFY`` on any bad wave,
        and ``na_last_error`` then names the first failing unit."""
        return self._matrix_sweep_verify("mfma", recs, outer, seed, dtype)

    def mfma_sweep(self, dev: int, dtype: str = "bf16", workgroups: int = 0, outer: int = 0,
                   seed: int = DEFAULT_MFMA_SWEEP_SEED) -> MfmaSweepResult:
        """Run one wave per SIMD on every CU through a long MFMA chain
        (``workgroups`` 0 = 4 per CU, ``outer`` 0 = the default fold count),
        verify every wave bit-exactly against the host reference, and
        report sustained TFLOP/s and the in-kernel clock. Wrong waves come
        back in the result (``.ok`` False) with the units they ran on, not
        as an exception. The TFLOP/s figure is on small-integer operands held
        in registers and is not comparable to GEMM benchmarks."""
        return self._matrix_sweep("mfma", dev, dtype, workgroups, outer, seed)

    def _run_mfma_sweep(self, g: GPUReport) -> None:
        for dtype in ("bf16", "fp8"):
            res = self.mfma_sweep(g.index, dtype)
            g.mfma_sweep_bad_waves += res.bad_waves
            if dtype == "bf16":
                g.mfma_sweep_tflops = round(res.tflops, 1)
                g.mfma_sweep_clock_mhz = round(res.clock_mhz, 1)
                g.mfma_sweep_units_seen = res.units_seen
                if res.tflops < MIN_MFMA_SWEEP_TFLOPS:
                    g.problems.append(
                        f"MFMA sweep bf16 {g.mfma_sweep_tflops} TFLOP/s below floor "
                        f"{MIN_MFMA_SWEEP_TFLOPS}"
                    )
            else:
                g.mfma_sweep_fp8_tflops = round(res.tflops, 1)
            if not res.ok:
                g.problems.append(f"MFMA sweep {dtype}: {res.describe()}")

    # -- chip-wide MX sweep ------------------------------------------------------

    def mx_sweep_expected(self, wave: int, outer: int, seed: int = DEFAULT_MX_SWEEP_SEED) -> int:
        """Checksum wave ``wave`` of the MX sweep must report after ``outer``
        folds, in either format (host arithmetic only; needs no GPU)."""
        return self._matrix_sweep_expected("mx", wave, outer, seed)

    def mx_sweep_run(self, dev: int, fmt: str = "fp4", workgroups: int = 1, outer: int = 1,
                     seed: int = DEFAULT_MX_SWEEP_SEED) -> tuple:
        """As ``mfma_sweep_run``, on v_mfma_scale_f32_16x16x128_f8f6f4 with
        operands in ``fmt`` ("fp4" = E2M1, "fp6" = E2M3) and scales of 1.0."""
        return self._matrix_sweep_run("mx", dev, fmt, workgroups, outer, seed)

    def mx_sweep_verify(self, recs, outer: int, seed: int = DEFAULT_MX_SWEEP_SEED,
                        fmt: str = "fp4") -> tuple:
        """As ``mfma_sweep_verify``, against the MX sweep's reference."""
        return self._matrix_sweep_verify("mx", recs, outer, seed, fmt)

    def mx_sweep(self, dev: int, fmt: str = "fp4", workgroups: int = 0, outer: int = 0,
                 seed: int = DEFAULT_MX_SWEEP_SEED) -> MfmaSweepResult:
        """As ``mfma_sweep``, on the block-scaled 16x16x128 instruction in
        ``fmt``: every SIMD of every CU issues fp4 / fp6 MFMAs, each wave
        checked bit-exactly. 65536 FLOP per MFMA; the TFLOP/s caveat of
        ``mfma_sweep`` applies."""
        return self._matrix_sweep("mx", dev, fmt, workgroups, outer, seed)

    def _run_mx_sweep(self, g: GPUReport) -> None:
        for fmt in MX_SWEEP_FORMATS:
            res = self.mx_sweep(g.index, fmt)
            g.mx_sweep_bad_waves += res.bad_waves
            setattr(g, f"mx_sweep_{fmt}_tflops", round(res.tflops, 1))
            if fmt == "fp4" and res.tflops < MIN_MX_SWEEP_TFLOPS:
                g.problems.append(
                    f"MX sweep fp4 {g.mx_sweep_fp4_tflops} TFLOP/s below floor "
                    f"{MIN_MX_SWEEP_TFLOPS}"
                )
            if not res.ok:
                g.problems.append(f"MX sweep {fmt}: {res.describe()}")

    # -- chip-wide LDS sweep ----------------------------------------------------

    def lds_sweep_allocation(self, dev: int) -> int:
        """Bytes of LDS a workgroup of the sweep holds, and tests when
        ``lds_bytes`` is 0: the device's per-workgroup maximum, at most
        160 KiB."""
        out = ctypes.c_longlong(0)
        rc = self.lib.na_lds_sweep_allocation(dev, ctypes.byref(out))
        self._check(rc, f"lds_sweep_allocation({dev})")
        return out.value

    def lds_sweep_expected(self, workgroup: int, lds_bytes: int, iters: int,
                           seed: int = DEFAULT_LDS_SWEEP_SEED) -> list:
        """The checksums workgroup ``workgroup`` must report, one per phase of
        ``LDS_SWEEP_PHASES``, testing ``lds_bytes`` (explicit here: a multiple
        of 4096 up to 160 KiB) with ``iters`` stream passes (host arithmetic
        only; needs no GPU)."""
        out = (ctypes.c_uint64 * len(LDS_SWEEP_PHASES))()
        rc = self.lib.na_lds_sweep_expected(seed, workgroup, lds_bytes, iters, out, len(out))
        self._check(rc, "lds_sweep_expected")
        return list(out)

    def lds_sweep_run(self, dev: int, workgroups: int = 1, lds_bytes: int = 0, iters: int = 1,
                      seed: int = DEFAULT_LDS_SWEEP_SEED) -> tuple:
        """One launch of ``workgroups`` workgroups, each through every phase
        on the leading ``lds_bytes`` of its LDS (0 = all of it) with ``iters``
        stream passes. Returns ``(records, ms)``: a ctypes array of
        ``LdsRecord`` (record i is workgroup i) and the HIP-event time."""
        return self._sweep_run(
            "lds_sweep_run", LdsRecord, max(workgroups, 0),
            dev, workgroups, lds_bytes, iters, seed,
        )

    def lds_sweep_verify(self, recs, lds_bytes: int, iters: int,
                         seed: int = DEFAULT_LDS_SWEEP_SEED) -> tuple:
        """Compare every record against the host reference (``lds_bytes``
        explicit, as for ``lds_sweep_expected``). Returns ``(rc,
        LdsSweepResult)``; rc is ``NA_ERR_VERIFY`` on any bad workgroup, and
        ``na_last_error`` then names the first failing phase and CU."""
        return self._sweep_verify(
            "lds_sweep_verify", recs, (lds_bytes, iters, seed), _LdsSweepResultC(),
            LdsSweepResult._from_c, LdsSweepResult,
        )

    def lds_sweep(self, dev: int, workgroups: int = 0, lds_bytes: int = 0, iters: int = 0,
                  seed: int = DEFAULT_LDS_SWEEP_SEED) -> LdsSweepResult:
        """Run one workgroup at a time on every CU through every LDS access
        path — 32- and 128-bit accesses, LDS-DMA at 16, 4 and 12 bytes, the
        transposed read, atomics — and a timed read stream (``workgroups`` 0
        = 4 per CU, ``lds_bytes`` 0 = the whole allocation, ``iters`` 0 = the
        default pass count), verify every phase of every workgroup bit-exactly
        against the host reference, and report the stream rate per CU and
        chip-wide. Wrong workgroups come back in the result (``.ok`` False)
        with the CUs they ran on, not as an exception."""
        res = _LdsSweepResultC()
        gbs = ctypes.c_double(0)
        rc = self.lib.na_lds_sweep(
            dev, workgroups, ctypes.c_longlong(lds_bytes), iters, ctypes.c_ulonglong(seed),
            ctypes.byref(res), ctypes.byref(gbs),
        )
        self._check(rc, f"lds_sweep({dev})", (NA_OK, NA_ERR_VERIFY))
        return LdsSweepResult._from_c(res, gbs.value)

    def _run_lds_sweep(self, g: GPUReport) -> None:
        res = self.lds_sweep(g.index)
        g.lds_sweep_gbs = round(res.gbs, 1)
        g.lds_sweep_min_cu_bytes_per_clk = round(res.min_bytes_per_clk, 2)
        g.lds_sweep_units_seen = res.units_seen
        g.lds_sweep_bad_workgroups = res.bad_workgroups
        if res.gbs < MIN_LDS_SWEEP_GBS:
            g.problems.append(
                f"LDS sweep {g.lds_sweep_gbs} GB/s below floor {MIN_LDS_SWEEP_GBS}"
            )
        if not res.ok:
            g.problems.append(f"LDS sweep: {res.describe()}")

    # -- chip-wide cache sweep ---------------------------------------------------

    def cache_sweep_expected(self, workgroup: int, workgroups: int, slice_bytes: int, iters: int,
                             seed: int = DEFAULT_CACHE_SWEEP_SEED) -> list:
        """The checksums workgroup ``workgroup`` of ``workgroups`` must
        report, one per phase of ``CACHE_SWEEP_PHASES``, on a slice of
        ``slice_bytes`` (a multiple of 4096 up to 1 MiB) with ``iters`` stream
        passes: all but the last in its record of the first launch, the last
        in that of the second (host arithmetic only; needs no GPU)."""
        out = (ctypes.c_uint64 * len(CACHE_SWEEP_PHASES))()
        rc = self.lib.na_cache_sweep_expected(
            seed, workgroup, workgroups, slice_bytes, iters, out, len(out))
        self._check(rc, "cache_sweep_expected")
        return list(out)

    def cache_sweep_run(self, dev: int, workgroups: int = 1, slice_bytes: int = 65536,
                        iters: int = 1, seed: int = DEFAULT_CACHE_SWEEP_SEED) -> tuple:
        """Both launches of ``workgroups`` workgroups, each on a slice of
        ``slice_bytes`` of device memory with ``iters`` stream passes. Returns
        ``(records, ms)``: a ctypes array of 2 x ``workgroups`` ``LdsRecord``
        (record i is workgroup i mod ``workgroups`` of launch i //
        ``workgroups``) and the HIP-event time of the pair."""
        return self._sweep_run(
            "cache_sweep_run", LdsRecord, 2 * max(workgroups, 0),
            dev, workgroups, slice_bytes, iters, seed,
        )

    def cache_sweep_verify(self, recs, slice_bytes: int, iters: int,
                           seed: int = DEFAULT_CACHE_SWEEP_SEED) -> tuple:
        """Compare the records of both launches against the host reference.
        Returns ``(rc, CacheSweepResult)``; rc is ``NA_ERR_VERIFY`` on any bad
        record, and ``na_last_error`` then names the first failing phase and
        CU, for ``xread`` also the CU that wrote the slice."""
        return self._sweep_verify(
            "cache_sweep_verify", recs, (slice_bytes, iters, seed), _LdsSweepResultC(),
            CacheSweepResult._from_c, CacheSweepResult,
        )

    def cache_sweep(self, dev: int, workgroups: int = 0, slice_bytes: int = 0, iters: int = 0,
                    seed: int = DEFAULT_CACHE_SWEEP_SEED) -> CacheSweepResult:
        """Run one workgroup at a time on every CU through what lies between
        a CU and HBM — the vector L1, the XCD's L2, write-through and refill,
        global atomics, the scalar data cache — and a timed read stream from
        the L2, then read every slice back from another workgroup, normally on
        another XCD (``workgroups`` 0 = 4 per CU, ``slice_bytes`` 0 = 64 KiB,
        ``iters`` 0 = the default pass count). Every phase of every workgroup
        is verified bit-exactly against the host reference. Wrong workgroups
        come back in the result (``.ok`` False) with the CUs they ran on, not
        as an exception."""
        res = _LdsSweepResultC()
        gbs = ctypes.c_double(0)
        rc = self.lib.na_cache_sweep(
            dev, workgroups, ctypes.c_longlong(slice_bytes), iters, ctypes.c_ulonglong(seed),
            ctypes.byref(res), ctypes.byref(gbs),
        )
        self._check(rc, f"cache_sweep({dev})", (NA_OK, NA_ERR_VERIFY))
        return CacheSweepResult._from_c(res, gbs.value)

    def _run_cache_sweep(self, g: GPUReport) -> None:
        res = self.cache_sweep(g.index)
        g.cache_sweep_gbs = round(res.gbs, 1)
        g.cache_sweep_min_cu_bytes_per_clk = round(res.min_bytes_per_clk, 2)
        g.cache_sweep_units_seen = res.units_seen
        g.cache_sweep_bad_workgroups = res.bad_workgroups
        if res.gbs < MIN_CACHE_SWEEP_GBS:
            g.problems.append(
                f"cache sweep: {g.cache_sweep_gbs} GB/s below floor {MIN_CACHE_SWEEP_GBS}"
            )
        if not res.ok:
            g.problems.append(f"cache sweep: {res.describe()}")

    # -- chip-wide vector-unit sweep ---------------------------------------------

    def valu_sweep_slots(self) -> int:
        """Registers per lane the register-file phases pattern-test."""
        return self.lib.na_valu_sweep_slots()

    def valu_sweep_xlane_table(self, move: int) -> list:
        """Source slot of every destination slot under cross-lane move
        ``move`` of the xlane phase, as the host reference models it: 64
        lanes, or for the two swaps 128 (A's lanes, then B's). Needs no GPU."""
        out = (ctypes.c_int * 128)()
        n = self.lib.na_valu_sweep_xlane_table(move, out, len(out))
        if n < 0:
            raise NodeAgentError(f"valu_sweep_xlane_table: {self._err()}")
        return list(out[:n])

    def valu_sweep_expected(self, wave: int, iters: int,
                            seed: int = DEFAULT_VALU_SWEEP_SEED) -> list:
        """The checksums wave ``wave`` must report, one per phase of
        ``VALU_SWEEP_PHASES``, with ``iters`` stream rounds; the ``trans``
        entry, which has no host reference, is 0 (host arithmetic only; needs
        no GPU)."""
        out = (ctypes.c_uint64 * len(VALU_SWEEP_PHASES))()
        rc = self.lib.na_valu_sweep_expected(seed, wave, iters, out)
        self._check(rc, "valu_sweep_expected")
        return list(out)

    def valu_sweep_run(self, dev: int, workgroups: int = 1, iters: int = 1,
                       seed: int = DEFAULT_VALU_SWEEP_SEED) -> tuple:
        """One launch of ``workgroups`` x 4 waves, each through every phase
        with ``iters`` stream rounds. Returns ``(records, ms)``: a ctypes
        array of ``ValuRecord`` (record i is wave i) and the HIP-event time."""
        return self._sweep_run(
            "valu_sweep_run", ValuRecord, max(workgroups, 0) * MFMA_SWEEP_WAVES_PER_WG,
            dev, workgroups, iters, seed,
        )

    def valu_sweep_verify(self, recs, iters: int, seed: int = DEFAULT_VALU_SWEEP_SEED) -> tuple:
        """Compare every record against the host reference and, for the
        transcendental phase, against the other records. Returns ``(rc,
        ValuSweepResult)``; rc is ``NA_ERR_VERIFY`` on any bad wave, and
        ``na_last_error`` then names the first failing unit and phase."""
        return self._sweep_verify(
            "valu_sweep_verify", recs, (iters, seed),
            _ValuSweepResultC(), ValuSweepResult._from_c, ValuSweepResult,
        )

    def valu_sweep(self, dev: int, workgroups: int = 0, iters: int = 0,
                   seed: int = DEFAULT_VALU_SWEEP_SEED) -> ValuSweepResult:
        """Run one wave per SIMD on every CU through the vector unit: a
        pattern over 480 of the 512 registers per lane at both polarities,
        integer, f32, f64, packed-f32/f16, cross-lane and transcendental
        chains, and a timed packed-f32 stream (``workgroups`` 0 = 4 per CU,
        ``iters`` 0 = the default round count). Every exact phase of every
        wave is verified bit for bit against the host reference, the
        transcendental phase by consensus among the SIMDs (a fault common to
        the whole chip passes it). Wrong waves come back in the result
        (``.ok`` False) with the SIMDs they ran on, not as an exception."""
        res = _ValuSweepResultC()
        rc = self.lib.na_valu_sweep(
            dev, workgroups, iters, ctypes.c_ulonglong(seed), ctypes.byref(res)
        )
        self._check(rc, f"valu_sweep({dev})", (NA_OK, NA_ERR_VERIFY))
        return ValuSweepResult._from_c(res)

    def _run_valu_sweep(self, g: GPUReport) -> None:
        res = self.valu_sweep(g.index)
        g.valu_sweep_tflops = round(res.tflops, 1)
        g.valu_sweep_min_simd_flop_per_clk = round(res.min_flop_per_clk, 2)
        g.valu_sweep_simds_seen = res.simds_seen
        g.valu_sweep_bad_waves = res.bad_waves
        g.valu_sweep_trans_unchecked = res.trans_unchecked
        if res.tflops < MIN_VALU_SWEEP_TFLOPS:
            g.problems.append(
                f"VALU sweep {g.valu_sweep_tflops} TFLOP/s below floor {MIN_VALU_SWEEP_TFLOPS}"
            )
        if not res.ok:
            g.problems.append(f"VALU sweep: {res.describe()}")

    # -- chip-wide load sweep ----------------------------------------------------

    def load_sweep_stream_expected(self, workgroup: int, slice_bytes: int, passes: int,
                                   seed: int = DEFAULT_LOAD_SWEEP_SEED) -> list:
        """The checksums the four stream waves of workgroup ``workgroup`` must
        report after ``passes`` passes over its slice of ``slice_bytes`` (a
        multiple of 16384 up to 16 MiB). The matrix waves' are
        ``mfma_sweep_expected`` of the same seed. Host arithmetic only; needs
        no GPU."""
        out = (ctypes.c_uint64 * MFMA_SWEEP_WAVES_PER_WG)()
        rc = self.lib.na_load_sweep_stream_expected(
            seed, workgroup, slice_bytes, passes, out, len(out))
        self._check(rc, "load_sweep_stream_expected")
        return list(out)

    def load_sweep_run(self, dev: int, region: int, workgroups: int = 1, outer: int = 1,
                       slice_bytes: int = LOAD_SWEEP_GRANULE, passes: int = 1,
                       seed: int = DEFAULT_LOAD_SWEEP_SEED, dtype: str = "bf16") -> tuple:
        """One launch of ``workgroups`` x 8 waves on the caller-owned device
        memory at ``region``: ``workgroups * slice_bytes`` bytes already
        filled through ``memtest_fill`` with the same seed. Four waves of a
        workgroup run ``outer`` folds of the matrix-core sweep's chain in
        ``dtype``, four stream its slice ``passes`` times through LDS and
        compare every word; ``outer`` 0 or ``passes`` 0 switches that role
        off. Returns ``(matrix, stream, mem, ms)``: two ctypes arrays of
        ``MfmaRecord`` (record i is wave i of its role), the stream waves' own
        comparison as a ``MemtestResult`` (a mismatch is reported there, not
        raised) and the HIP-event time."""
        n = max(workgroups, 0) * MFMA_SWEEP_WAVES_PER_WG
        matrix, stream = (MfmaRecord * max(n, 1))(), (MfmaRecord * max(n, 1))()
        mem, ms = _MemtestResultC(), ctypes.c_double(0)
        rc = self.lib.na_load_sweep_run(
            dev, self._matrix_code("mfma", dtype), workgroups, outer, region, slice_bytes, passes,
            seed, matrix, stream, n, ctypes.byref(mem), ctypes.byref(ms))
        self._check(rc, f"load_sweep_run({dev})", (NA_OK, NA_ERR_VERIFY))
        return matrix, stream, MemtestResult(**_shared_fields(MemtestResult, mem)), ms.value

    def load_sweep_verify(self, matrix, stream, outer: int, slice_bytes: int, passes: int,
                          seed: int = DEFAULT_LOAD_SWEEP_SEED, dtype: str = "bf16") -> tuple:
        """Compare the records of both roles against the host references.
        Returns ``(rc, LoadSweepResult)``; rc is ``NA_ERR_VERIFY`` on any bad
        wave, and ``na_last_error`` then names the role and unit of the
        first. The records of a role that was off must be all zero."""
        res_m, res_s = _MfmaSweepResultC(), _MfmaSweepResultC()
        rc = self.lib.na_load_sweep_verify(
            matrix, stream, len(matrix), outer, slice_bytes, passes, seed,
            ctypes.byref(res_m), ctypes.byref(res_s))
        if rc not in (NA_OK, NA_ERR_VERIFY):
            return rc, LoadSweepResult()
        return rc, LoadSweepResult(MfmaSweepResult._from_c(dtype, res_m),
                                   MfmaSweepResult._from_c(dtype, res_s))

    def load_sweep(self, dev: int, dtype: str = "bf16", workgroups: int = 0, outer: int = 0,
                   slice_bytes: int = 0, passes: int = 0,
                   seed: int = DEFAULT_LOAD_SWEEP_SEED) -> LoadSweepResult:
        """Run one workgroup of eight waves at a time on every CU, two waves
        per SIMD: four on the matrix-core sweep's MFMA chain, four streaming
        a slice of pattern-filled device memory through LDS and comparing
        every word, so that matrix cores, LDS and HBM are busy in the same
        cycles (0 = the default for ``workgroups``, 4 per CU, and for
        ``outer``, ``slice_bytes``, 4 MiB, and ``passes``). Every wave is
        verified bit-exactly against the host references. Wrong waves and
        words come back in the result (``.ok`` False) with the units they ran
        on, not as an exception; a region that does not fit in half of the
        free device memory raises ``LoadSweepNoRoom``."""
        res_m, res_s, mem = _MfmaSweepResultC(), _MfmaSweepResultC(), _MemtestResultC()
        tflops, gbs, overlap = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        rc = self.lib.na_load_sweep(
            dev, self._matrix_code("mfma", dtype), workgroups, outer,
            ctypes.c_longlong(slice_bytes), passes, ctypes.c_ulonglong(seed), ctypes.byref(res_m),
            ctypes.byref(res_s), ctypes.byref(mem), ctypes.byref(tflops), ctypes.byref(gbs),
            ctypes.byref(overlap),
        )
        if rc not in (NA_OK, NA_ERR_VERIFY):
            err = self._err()
            cls = LoadSweepNoRoom if "does not fit" in err else NodeAgentError
            raise cls(f"load_sweep({dev}): {err}")
        return LoadSweepResult(
            MfmaSweepResult._from_c(dtype, res_m), MfmaSweepResult._from_c(dtype, res_s),
            MemtestResult(**_shared_fields(MemtestResult, mem)),
            tflops.value, gbs.value, overlap.value,
        )

    def _run_load_sweep(self, g: GPUReport) -> None:
        try:
            res = self.load_sweep(g.index)
        except LoadSweepNoRoom as e:
            # a busy GPU must not get its node replaced for lack of free memory
            g.load_sweep_skipped = str(e)
            return
        g.load_sweep_tflops = round(res.tflops, 1)
        g.load_sweep_gbs = round(res.gbs, 1)
        g.load_sweep_clock_mhz = round(res.matrix.clock_mhz, 1)
        g.load_sweep_overlap = round(res.overlap, 3)
        g.load_sweep_units_seen = res.matrix.units_seen
        g.load_sweep_bad_waves = res.matrix.bad_waves + res.stream.bad_waves
        g.load_sweep_bad_words = res.mem.bad_words
        if res.tflops < MIN_LOAD_SWEEP_TFLOPS:
            g.problems.append(
                f"load sweep {g.load_sweep_tflops} TFLOP/s below floor {MIN_LOAD_SWEEP_TFLOPS}"
            )
        if res.gbs < MIN_LOAD_SWEEP_GBS:
            g.problems.append(
                f"load sweep {g.load_sweep_gbs} GB/s below floor {MIN_LOAD_SWEEP_GBS}"
            )
        if not res.ok:
            g.problems.append(f"load sweep: {res.describe()}")

    def p2p_matrix(self, n: int) -> list:
        buf = (ctypes.c_int * (n * n))()
        self._check(self.lib.na_p2p_matrix(n, buf), "p2p_matrix")
        return [[buf[i * n + j] for j in range(n)] for i in range(n)]

    def p2p_bandwidth(self, src: int, dst: int, bytes_: int = 256 << 20, iters: int = 5) -> float:
        out = ctypes.c_double(0)
        rc = self.lib.na_p2p_bandwidth(src, dst, bytes_, iters, ctypes.byref(out))
        self._check(rc, f"p2p_bandwidth({src},{dst})")
        return out.value

    # -- full health check ---------------------------------------------------

    def check(self, expect_gpus: int = 0, bw_bytes: int = 1 << 30,
              memtest_bytes: int = 0, mfma_sweep: bool = False, mx_checks: bool = False,
              mx_sweep: bool = False, lds_sweep: bool = False,
              valu_sweep: bool = False, cache_sweep: bool = False,
              load_sweep: bool = False) -> NodeReport:
        """Full health battery. ``memtest_bytes`` > 0 additionally runs the
        HBM data-integrity test on that many bytes per GPU, clamped to 90 %
        of what the device reports free; if nothing can be allocated the
        reason lands in ``hbm_memtest_skipped`` and the GPU stays healthy.
        Regions under 512 MiB are allowed but are served largely from the
        256 MiB Infinity Cache, not DRAM. 0 (default) runs nothing new.

        ``mfma_sweep`` additionally runs the chip-wide matrix-core sweep in
        bf16 and fp8 on every GPU: a wrong wave is a problem that names the
        unit it ran on, as is a bf16 rate under ``MIN_MFMA_SWEEP_TFLOPS``.
        ``mfma_sweep_units_seen`` below the CU count is reported, not a
        problem. False (default) makes no sweep call.

        ``mx_checks`` additionally runs the single-wave MX checks of
        ``MX_CHECK_KINDS`` (fp4, fp6, bf6, bf8 and mixed operands, per-lane
        scales, scale byte select) on every GPU; a failed kind is a problem
        that carries the first wrong word. ``mx_sweep`` additionally runs the
        chip-wide sweep on the block-scaled instruction in fp4 and fp6: a
        wrong wave is a problem that names its unit, as is an fp4 rate under
        ``MIN_MX_SWEEP_TFLOPS``. False (default) calls nothing new.

        ``lds_sweep`` additionally runs the chip-wide LDS sweep on every GPU:
        a wrong workgroup is a problem that names its CU and the phase that
        failed, as is a stream rate under ``MIN_LDS_SWEEP_GBS``.
        ``lds_sweep_units_seen`` below the CU count is reported, not a
        problem. False (default) makes no new library call.

        ``valu_sweep`` additionally runs the chip-wide vector-unit sweep on
        every GPU: a wrong wave is a problem that names its SIMD and the
        phases that failed, as is a stream rate under
        ``MIN_VALU_SWEEP_TFLOPS``. ``valu_sweep_simds_seen`` below 4 x the CU
        count and ``valu_sweep_trans_unchecked`` are reported, not problems.
        False (default) makes no new library call.

        ``cache_sweep`` additionally runs the chip-wide cache sweep on every
        GPU: a wrong workgroup is a problem that names its CU and the phase
        that failed (or the XCC whose L2 is suspect), as is a stream rate
        under ``MIN_CACHE_SWEEP_GBS``. ``cache_sweep_units_seen`` below the CU
        count is reported, not a problem. False (default) makes no new
        library call.

        ``load_sweep`` additionally runs the chip-wide load sweep on every
        GPU: matrix cores, LDS and HBM of every CU busy in the same cycles. A
        wrong matrix or stream wave is a problem that names its role and unit
        and says that it failed under combined load, as are a mismatch seen
        by the stream waves' own comparison and a rate under
        ``MIN_LOAD_SWEEP_TFLOPS`` or ``MIN_LOAD_SWEEP_GBS``. If the region
        does not fit in half of the free device memory the reason lands in
        ``load_sweep_skipped`` and the GPU stays healthy;
        ``load_sweep_units_seen`` below the CU count is reported, not a
        problem. False (default) makes no new library call."""
        report = NodeReport()
        report.gpu_count = self.device_count()
        if expect_gpus and report.gpu_count != expect_gpus:
            report.problems.append(
                f"expected {expect_gpus} GPUs, found {report.gpu_count}"
            )
        for d in range(report.gpu_count):
            g = GPUReport(index=d)
            try:
                g.name, g.arch, hbm, g.cus = self.device_info(d)
                g.hbm_gb = round(hbm / 1e9, 1)
                if EXPECTED_ARCH not in g.arch:
                    g.problems.append(f"arch {g.arch} != {EXPECTED_ARCH}")
                g.hbm_bw_gbs = round(self.hbm_bandwidth(d, bw_bytes), 1)
                if g.hbm_bw_gbs < MIN_HBM_BW_GBS:
                    g.problems.append(
                        f"HBM bandwidth {g.hbm_bw_gbs} GB/s below floor {MIN_HBM_BW_GBS}"
                    )
                for method, report_field, label in _SELFTESTS:
                    ok = getattr(self, method)(d)
                    if method == "lds_selftest":
                        ok, g.lds_bytes_tested = ok
                    if report_field:
                        setattr(g, report_field, ok)
                    if not ok:
                        g.problems.append(f"{label} failed: {self._err()}")
                g.sdma_bw_gbs = round(self.sdma_bandwidth(d), 1)
                if g.sdma_bw_gbs < MIN_SDMA_BW_GBS:
                    g.problems.append(
                        f"SDMA D2D bandwidth {g.sdma_bw_gbs} GB/s below floor {MIN_SDMA_BW_GBS}"
                    )
                if memtest_bytes > 0:
                    self._run_memtest(g, memtest_bytes)
                if mfma_sweep:
                    self._run_mfma_sweep(g)
                if mx_checks:
                    self._run_mx_checks(g)
                if mx_sweep:
                    self._run_mx_sweep(g)
                if lds_sweep:
                    self._run_lds_sweep(g)
                if cache_sweep:
                    self._run_cache_sweep(g)
                if valu_sweep:
                    self._run_valu_sweep(g)
                if load_sweep:
                    self._run_load_sweep(g)
            except NodeAgentError as e:
                g.problems.append(str(e))
            g.healthy = not g.problems
            report.gpus.append(g)
        if report.gpu_count > 1:
            report.xgmi_p2p = self.p2p_matrix(report.gpu_count)
            for i in range(report.gpu_count):
                for j in range(report.gpu_count):
                    if i != j and not report.xgmi_p2p[i][j]:
                        report.problems.append(f"no xGMI peer access {i}->{j}")
        report.problems.extend(
            p for g in report.gpus for p in (f"gpu{g.index}: {q}" for q in g.problems)
        )
        report.healthy = not report.problems and report.gpu_count > 0
        return report


# -- node condition publishing (the repair feedback loop) --------------------
#
# The DaemonSet runs the check in a loop and publishes the result as the
# AMDGPUHealthy condition on its Node. The cloud provider's RepairPolicies
# include (AMDGPUHealthy, False, 5 min), so the node.health controller
# replaces nodes with failed HBM/MFMA/LDS/xGMI self-tests — on-node GPU
# evidence the reference's NodeReady-only repair can't see.


def node_condition_from_report(report: NodeReport) -> dict:
    from .apis import v1 as karpv1

    if report.healthy:
        return {
            "type": karpv1.AMD_GPU_HEALTHY_CONDITION_TYPE,
            "status": "True",
            "reason": "AllChecksPassed",
            "message": f"{report.gpu_count} GPU(s) passed HBM/FMA/MFMA/LDS/xGMI self-tests",
        }
    return {
        "type": karpv1.AMD_GPU_HEALTHY_CONDITION_TYPE,
        "status": "False",
        "reason": "GPUUnhealthy",
        "message": "; ".join(report.problems)[:1024] or "node agent found no GPUs",
    }


async def patch_node_condition(kube, node_name: str, report: NodeReport) -> None:
    """Merge the AMDGPUHealthy condition into the Node's status conditions.

    The status write carries the read's resourceVersion as an optimistic
    lock and retries on conflict: a merge patch of the full conditions list
    from an unconditioned GET races the kubelet's concurrent status writes
    and can clobber or resurrect kubelet-owned conditions (the same
    lost-update class TerminationController._set_nodeclaim_condition guards
    against)."""
    from .kube import objects as ko
    from .kube.client import ConflictError

    cond = node_condition_from_report(report)
    for _ in range(5):
        node = await kube.get("v1", "Node", node_name)
        ko.set_condition(node, cond["type"], cond["status"], cond["reason"], cond["message"])
        try:
            await kube.patch(
                "v1",
                "Node",
                node_name,
                {
                    "metadata": {
                        "resourceVersion": node.get("metadata", {}).get("resourceVersion")
                    },
                    "status": {"conditions": node["status"]["conditions"]},
                },
                subresource="status",
            )
            return
        except ConflictError:
            continue
    raise NodeAgentError(
        f"node {node_name}: AMDGPUHealthy condition patch abandoned after repeated conflicts"
    )


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="MI355X node health agent")
    ap.add_argument("--json", action="store_true", help="emit JSON report")
    ap.add_argument("--expect-gpus", type=int, default=0)
    ap.add_argument("--bw-bytes", type=int, default=1 << 30)
    ap.add_argument(
        "--memtest-bytes",
        type=int,
        default=0,
        metavar="N",
        help="also pattern-test N bytes of HBM per GPU (fill / verify+invert / verify), "
        "clamped to 90%% of free device memory; 0 = off. Regions under 512 MiB are "
        "allowed but are served largely from the 256 MiB Infinity Cache, not DRAM",
    )
    ap.add_argument(
        "--mfma-sweep",
        action="store_true",
        help="also run the chip-wide matrix-core sweep on every GPU: one wave per SIMD of "
        "every CU through a long bf16 and fp8 MFMA chain, each wave checked bit-exactly and "
        "a wrong one attributed to its XCC/SE/SH/CU/SIMD; reports sustained TFLOP/s "
        "(integer operands: not comparable to GEMM benchmarks) and the in-kernel clock",
    )
    ap.add_argument(
        "--mx-checks",
        action="store_true",
        help="also run the single-wave checks of the block-scaled MX matrix instructions: "
        "fp4, fp6, bf6, bf8 and fp8 x fp4 operands, per-lane E8M0 scales, every scale byte "
        "select, both tile shapes, and every code point of the sub-byte formats",
    )
    ap.add_argument(
        "--mx-sweep",
        action="store_true",
        help="also run the chip-wide sweep on the block-scaled 16x16x128 instruction in fp4 "
        "and fp6 on every GPU: as --mfma-sweep, each wave checked bit-exactly and a wrong one "
        "attributed to its XCC/SE/SH/CU/SIMD; reports sustained TFLOP/s per format",
    )
    ap.add_argument(
        "--lds-sweep",
        action="store_true",
        help="also run the chip-wide LDS sweep on every GPU: one workgroup at a time on every "
        "CU through 32/128-bit accesses, LDS-DMA loads at 16/4/12 bytes, the transposed read "
        "and atomics, every phase checked bit-exactly and a wrong one attributed to its "
        "XCC/SE/SH/CU; reports the read-stream rate chip-wide and of the slowest CU",
    )
    ap.add_argument(
        "--cache-sweep",
        action="store_true",
        help="also run the chip-wide cache sweep on every GPU: one workgroup at a time on "
        "every CU, each on a cache-resident slice of device memory, through the vector L1, the "
        "XCD's L2, write-through and refill, global atomics and the scalar data cache, then "
        "every slice read back from another XCD; every phase checked bit-exactly and a wrong "
        "one attributed to its XCC/SE/SH/CU; reports the L2 read-stream rate chip-wide and of "
        "the slowest CU",
    )
    ap.add_argument(
        "--valu-sweep",
        action="store_true",
        help="also run the chip-wide vector-unit sweep on every GPU: one wave per SIMD of "
        "every CU through a register-file pattern (480 of 512 registers per lane, both "
        "polarities), integer, f32, f64, packed, cross-lane and transcendental chains, every "
        "exact phase checked bit for bit and a wrong one attributed to its "
        "XCC/SE/SH/CU/SIMD; reports the packed-f32 stream rate chip-wide and of the slowest SIMD",
    )
    ap.add_argument(
        "--load-sweep",
        action="store_true",
        help="also run the chip-wide load sweep on every GPU: one workgroup of eight waves at a "
        "time on every CU, four on the matrix-core sweep's bf16 MFMA chain while the other four "
        "stream a 4 MiB slice of pattern-filled HBM through LDS and compare every word, so that "
        "matrix cores, LDS and HBM are busy in the same cycles; every wave checked bit-exactly "
        "and a wrong one attributed to its role and XCC/SE/SH/CU/SIMD; reports the rates both "
        "roles reach together and the clock under that load",
    )
    ap.add_argument(
        "--patch-node",
        default="",
        metavar="NODE",
        help="publish the AMDGPUHealthy condition on this Node (in-cluster)",
    )
    args = ap.parse_args(argv)
    try:
        agent = NodeAgent()
        report = agent.check(
            expect_gpus=args.expect_gpus,
            bw_bytes=args.bw_bytes,
            memtest_bytes=args.memtest_bytes,
            mfma_sweep=args.mfma_sweep,
            mx_checks=args.mx_checks,
            mx_sweep=args.mx_sweep,
            lds_sweep=args.lds_sweep,
            valu_sweep=args.valu_sweep,
            cache_sweep=args.cache_sweep,
            load_sweep=args.load_sweep,
        )
    except NodeAgentError as e:
        print(json.dumps({"healthy": False, "agent_error": str(e)}))
        return 2
    if args.patch_node:
        import asyncio

        from .kube.http import HTTPClient

        async def publish():
            kube = HTTPClient.from_service_account()
            try:
                await patch_node_condition(kube, args.patch_node, report)
            finally:
                await kube.close()

        try:
            asyncio.run(publish())
        except Exception as e:
            print(json.dumps({"healthy": report.healthy, "patch_error": str(e)}))
            return 2
    out = asdict(report)
    if args.json:
        print(json.dumps(out, indent=2))
    else:
        print(json.dumps(out))
    return 0 if report.healthy else 1


if __name__ == "__main__":
    sys.exit(main())
