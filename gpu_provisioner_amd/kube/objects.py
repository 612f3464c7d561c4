"""Kubernetes object model: typed wrappers over the wire-format JSON dicts.

The store/client layer (kube/client.py, fake/apiserver.py) speaks plain JSON
dicts exactly as the kube-apiserver does; this module provides the typed
accessors controllers use. Mirrors the subset of apimachinery the reference
exercises (ObjectMeta, Conditions, OwnerReferences, Taints, resource
quantities) — see reference vendor/sigs.k8s.io/karpenter/pkg/apis/v1 for the
behavioral spec.
"""
from __future__ import annotations

import os
import re
import uuid
from dataclasses import dataclass
from fractions import Fraction
from datetime import datetime, timezone
from typing import Iterable, Optional

# ---------------------------------------------------------------------------
# time helpers (RFC3339, as the apiserver emits)
# ---------------------------------------------------------------------------


def now() -> datetime:
    return datetime.now(timezone.utc)


def _py_fmt_time(t: datetime) -> str:
    t = t.astimezone(timezone.utc)
    # hand-rolled RFC3339: strftime was measurable on the provision path
    return f"{t.year:04d}-{t.month:02d}-{t.day:02d}T{t.hour:02d}:{t.minute:02d}:{t.second:02d}Z"


def _py_fmt_micro_time(t: datetime) -> str:
    """metav1.MicroTime — Leases carry renew times at microsecond precision;
    whole-second truncation makes short leases look expired to followers."""
    t = t.astimezone(timezone.utc)
    return (
        f"{t.year:04d}-{t.month:02d}-{t.day:02d}T"
        f"{t.hour:02d}:{t.minute:02d}:{t.second:02d}.{t.microsecond:06d}Z"
    )


def parse_time(s: str) -> datetime:
    # Tolerate fractional seconds and explicit offsets.
    s = s.strip()
    if s.endswith("Z"):
        s = s[:-1] + "+00:00"
    return datetime.fromisoformat(s)


# ---------------------------------------------------------------------------
# resource.Quantity — the subset of kubernetes quantity arithmetic we need
# (parsing, comparison, formatting). Supports plain ints/floats, decimal SI
# suffixes (k, M, G, T, P, m for milli) and binary suffixes (Ki..Pi).
# ---------------------------------------------------------------------------

_QTY_RE = re.compile(r"^([+-]?[0-9]*\.?[0-9]+)([a-zA-Z]*)$")
_SUFFIX = {
    "": 1,
    "m": Fraction(1, 1000),
    "k": 10**3,
    "M": 10**6,
    "G": 10**9,
    "T": 10**12,
    "P": 10**15,
    "E": 10**18,
    "Ki": 2**10,
    "Mi": 2**20,
    "Gi": 2**30,
    "Ti": 2**40,
    "Pi": 2**50,
    "Ei": 2**60,
}


class _PyQuantity:
    """A kubernetes resource quantity. Immutable; compares by numeric value.

    Arithmetic is EXACT (Fraction, like upstream resource.Quantity's
    inf.Dec): float rounding on milli-quantities would make
    allocatable-precompute results drift from what the kubelet reports."""

    __slots__ = ("raw", "value")

    def __init__(self, raw: "str | int | float | Fraction | Quantity"):
        if isinstance(raw, _PyQuantity):
            self.raw, self.value = raw.raw, raw.value
            return
        if isinstance(raw, Fraction):
            self.value = raw
            self.raw = _fmt_num(raw)
            return
        if isinstance(raw, (int, float)):
            self.raw = str(raw)
            self.value = Fraction(raw)
            return
        m = _QTY_RE.match(str(raw))
        if not m:
            raise ValueError(f"invalid quantity {raw!r}")
        num, suf = m.groups()
        if suf not in _SUFFIX:
            raise ValueError(f"invalid quantity suffix {suf!r} in {raw!r}")
        self.raw = str(raw)
        self.value = Fraction(num) * _SUFFIX[suf]

    def __repr__(self) -> str:
        return f"Quantity({self.raw!r})"

    def __str__(self) -> str:
        return self.raw

    def __eq__(self, other: object) -> bool:
        return isinstance(other, _PyQuantity) and self.value == other.value

    def __lt__(self, other: "Quantity") -> bool:
        return self.value < other.value

    def __le__(self, other: "Quantity") -> bool:
        return self.value <= other.value

    def __hash__(self) -> int:
        return hash(self.value)

    def __add__(self, other: "Quantity") -> "Quantity":
        return _PyQuantity(self.value + other.value)

    def __sub__(self, other: "Quantity") -> "Quantity":
        return _PyQuantity(self.value - other.value)

    def is_zero(self) -> bool:
        return self.value == 0


def _fmt_num(v: Fraction) -> str:
    if v.denominator == 1:
        return str(v.numerator)
    milli = v * 1000
    if milli.denominator == 1:
        return f"{milli.numerator}m"  # sub-unit results render as milli
    return str(float(v))


class _NativeQuantity:
    """Quantity with the same surface as the class above, kept as an exact
    integer (numerator, denominator) pair in lowest terms. The native module
    parses, adds, subtracts and formats on that pair; `value` builds the
    Fraction only when it is read. Input the native parser does not cover
    (and any value beyond 64 bits) takes the class above's route, so results
    and error texts are its own."""

    __slots__ = ("raw", "_num", "_den", "_frac")

    def __init__(self, raw: "str | int | float | Fraction | Quantity"):
        t = type(raw)
        if t is str:
            pair = _native_objmodel.qty_parse(raw)
            if pair is not None:
                self.raw = raw
                self._num, self._den = pair
                self._frac = None
                return
        elif t is int:
            self.raw = str(raw)
            self._num, self._den, self._frac = raw, 1, None
            return
        elif t is _NativeQuantity:
            self.raw, self._num, self._den, self._frac = raw.raw, raw._num, raw._den, raw._frac
            return
        ref = _PyQuantity(raw)
        self.raw = ref.raw
        self._frac = v = ref.value
        self._num, self._den = v.numerator, v.denominator

    @classmethod
    def _of(cls, num: int, den: int, raw: str) -> "_NativeQuantity":
        q = cls.__new__(cls)
        q._num, q._den, q.raw, q._frac = num, den, raw, None
        return q

    @property
    def value(self) -> Fraction:
        v = self._frac
        if v is None:
            v = self._frac = Fraction(self._num, self._den)
        return v

    def __repr__(self) -> str:
        return f"Quantity({self.raw!r})"

    def __str__(self) -> str:
        return self.raw

    def __eq__(self, other: object) -> bool:
        return (
            isinstance(other, _NativeQuantity)
            and self._num == other._num
            and self._den == other._den
        )

    def __lt__(self, other: "Quantity") -> bool:
        return self._num * other._den < other._num * self._den

    def __le__(self, other: "Quantity") -> bool:
        return self._num * other._den <= other._num * self._den

    def __hash__(self) -> int:
        # hash(Fraction(n, 1)) == hash(n)
        return hash(self._num) if self._den == 1 else hash(self.value)

    def __add__(self, other: "Quantity") -> "Quantity":
        r = _native_objmodel.qty_addsub(self._num, self._den, other._num, other._den, False)
        return _NativeQuantity._of(*r) if r is not None else _NativeQuantity(self.value + other.value)

    def __sub__(self, other: "Quantity") -> "Quantity":
        r = _native_objmodel.qty_addsub(self._num, self._den, other._num, other._den, True)
        return _NativeQuantity._of(*r) if r is not None else _NativeQuantity(self.value - other.value)

    def is_zero(self) -> bool:
        return self._num == 0


def qty(v: "str | int | float | Quantity") -> "Quantity":
    return Quantity(v)


# ---------------------------------------------------------------------------
# ObjectMeta-level helpers over plain dict objects
# ---------------------------------------------------------------------------


def meta(obj: dict) -> dict:
    return obj.setdefault("metadata", {})


def _py_name_of(obj: dict) -> str:
    return obj.get("metadata", {}).get("name", "")


def _py_namespace_of(obj: dict) -> str:
    return obj.get("metadata", {}).get("namespace", "")


def _py_uid_of(obj: dict) -> str:
    return obj.get("metadata", {}).get("uid", "")


def _py_labels_of(obj: dict) -> dict:
    return obj.get("metadata", {}).get("labels") or {}


def _py_annotations_of(obj: dict) -> dict:
    return obj.get("metadata", {}).get("annotations") or {}


def set_label(obj: dict, key: str, value: str) -> None:
    meta(obj).setdefault("labels", {})[key] = value


def set_annotation(obj: dict, key: str, value: str) -> None:
    meta(obj).setdefault("annotations", {})[key] = value


def _py_finalizers_of(obj: dict) -> list:
    return obj.get("metadata", {}).get("finalizers") or []


def _py_has_finalizer(obj: dict, fin: str) -> bool:
    return fin in _py_finalizers_of(obj)


def add_finalizer(obj: dict, fin: str) -> bool:
    fins = meta(obj).setdefault("finalizers", [])
    if fin in fins:
        return False
    fins.append(fin)
    return True


def remove_finalizer(obj: dict, fin: str) -> bool:
    fins = meta(obj).get("finalizers") or []
    if fin not in fins:
        return False
    fins.remove(fin)
    return True


def deletion_timestamp_of(obj: dict) -> Optional[datetime]:
    ts = obj.get("metadata", {}).get("deletionTimestamp")
    return parse_time(ts) if ts else None


def creation_timestamp_of(obj: dict) -> Optional[datetime]:
    ts = obj.get("metadata", {}).get("creationTimestamp")
    return parse_time(ts) if ts else None


def _py_is_deleting(obj: dict) -> bool:
    return bool(obj.get("metadata", {}).get("deletionTimestamp"))


def _py_owner_references_of(obj: dict) -> list:
    return obj.get("metadata", {}).get("ownerReferences") or []


def set_owner_reference(obj: dict, owner: dict, *, block_deletion: bool = True) -> None:
    """Add/replace an owner reference pointing at `owner` (a full object dict)."""
    ref = {
        "apiVersion": owner.get("apiVersion", ""),
        "kind": owner.get("kind", ""),
        "name": name_of(owner),
        "uid": uid_of(owner),
        "blockOwnerDeletion": block_deletion,
    }
    refs = [r for r in owner_references_of(obj) if r.get("uid") != ref["uid"]]
    refs.append(ref)
    meta(obj)["ownerReferences"] = refs


# ---------------------------------------------------------------------------
# Conditions (metav1.Condition semantics: type/status/reason/message/
# lastTransitionTime/observedGeneration)
# ---------------------------------------------------------------------------

CONDITION_TRUE = "True"
CONDITION_FALSE = "False"
CONDITION_UNKNOWN = "Unknown"


def _py_get_condition(obj: dict, cond_type: str) -> Optional[dict]:
    for c in obj.get("status", {}).get("conditions") or []:
        if c.get("type") == cond_type:
            return c
    return None


def _py_condition_is(obj: dict, cond_type: str, status: str) -> bool:
    c = _py_get_condition(obj, cond_type)
    return bool(c) and c.get("status") == status


def _py_condition_is_true(obj: dict, cond_type: str) -> bool:
    return _py_condition_is(obj, cond_type, CONDITION_TRUE)


def _py_set_condition(
    obj: dict,
    cond_type: str,
    status: str,
    reason: str = "",
    message: str = "",
    *,
    at: Optional[datetime] = None,
) -> bool:
    """Set a condition; updates lastTransitionTime only on status change.

    Returns True if anything changed.
    """
    conds = obj.setdefault("status", {}).setdefault("conditions", [])
    existing = None
    for c in conds:
        if c.get("type") == cond_type:
            existing = c
            break
    ts = _py_fmt_time(at or now())
    if existing is None:
        conds.append(
            {
                "type": cond_type,
                "status": status,
                "reason": reason or status,
                "message": message,
                "lastTransitionTime": ts,
                "observedGeneration": obj.get("metadata", {}).get("generation", 0),
            }
        )
        return True
    changed = False
    if existing.get("status") != status:
        existing["status"] = status
        existing["lastTransitionTime"] = ts
        changed = True
    if reason and existing.get("reason") != reason:
        existing["reason"] = reason
        changed = True
    if existing.get("message") != message:
        existing["message"] = message
        changed = True
    existing["observedGeneration"] = obj.get("metadata", {}).get("generation", 0)
    return changed


# ---------------------------------------------------------------------------
# Node helpers (corev1.Node subset)
# ---------------------------------------------------------------------------


def _py_node_is_ready(node: dict) -> bool:
    for c in node.get("status", {}).get("conditions") or []:
        if c.get("type") == "Ready":
            return c.get("status") == CONDITION_TRUE
    return False


def _py_node_ready_condition(node: dict) -> Optional[dict]:
    for c in node.get("status", {}).get("conditions") or []:
        if c.get("type") == "Ready":
            return c
    return None


def node_taints(node: dict) -> list:
    return node.get("spec", {}).get("taints") or []


def node_allocatable(node: dict) -> dict:
    return node.get("status", {}).get("allocatable") or {}


def node_capacity(node: dict) -> dict:
    return node.get("status", {}).get("capacity") or {}


def _py_provider_id_of(node: dict) -> str:
    return node.get("spec", {}).get("providerID", "")


# ---------------------------------------------------------------------------
# Taints
# ---------------------------------------------------------------------------


@dataclass(frozen=True)
class Taint:
    key: str
    effect: str
    value: str = ""

    @classmethod
    def from_dict(cls, d: dict) -> "Taint":
        return cls(key=d.get("key", ""), effect=d.get("effect", ""), value=d.get("value", ""))

    def to_dict(self) -> dict:
        d = {"key": self.key, "effect": self.effect}
        if self.value:
            d["value"] = self.value
        return d

    def matches(self, other: "Taint") -> bool:
        return self.key == other.key and self.effect == other.effect


def merge_taints(existing: Iterable[dict], desired: Iterable[dict]) -> list:
    """Merge `desired` taints into `existing` (key+effect identity), keeping
    existing entries and appending missing desired ones — the semantics of
    karpenter's scheduling.Taints.Merge (reference vendor/.../pkg/scheduling/taints.go).
    """
    out = [dict(t) for t in existing]
    have = {(t.get("key"), t.get("effect")) for t in out}
    for t in desired:
        if (t.get("key"), t.get("effect")) not in have:
            out.append(dict(t))
            have.add((t.get("key"), t.get("effect")))
    return out


# ---------------------------------------------------------------------------
# misc
# ---------------------------------------------------------------------------


def _py_deep_copy(obj):
    """Fast deep copy for wire-format objects (pure JSON trees: dict/list/
    scalars). ~8× faster than copy.deepcopy, which dominated the provision
    path profile (49% of bench runtime) before this. Scalar leaves are
    returned without a recursive call — they are immutable."""
    t = type(obj)
    if t is dict:
        return {
            k: (_py_deep_copy(v) if type(v) is dict or type(v) is list else v)
            for k, v in obj.items()
        }
    if t is list:
        return [_py_deep_copy(v) if type(v) is dict or type(v) is list else v for v in obj]
    return obj


# The native JSON-tree extension (native/jsontree.cpp) replaces the tree
# walks when it has been built; the Python bodies stay as the fallback and
# as the reference the tests compare against. GPU_PROVISIONER_PURE_PYTHON=1
# forces the fallback. NATIVE_JSONTREE tells which path is live.
_native_jsontree = None
if os.environ.get("GPU_PROVISIONER_PURE_PYTHON") != "1":
    try:
        from .._native import _jsontree as _native_jsontree  # type: ignore
    except ImportError:
        _native_jsontree = None
NATIVE_JSONTREE = _native_jsontree is not None

deep_copy = _native_jsontree.deep_copy if NATIVE_JSONTREE else _py_deep_copy


def _py_now_rfc3339() -> str:
    """fmt_time(now()). The native version keeps the string of the current
    second, so calls within one second return the same object."""
    return _py_fmt_time(now())


def _py_uuid4_str() -> str:
    return str(uuid.uuid4())


# The native object-model extension (native/objmodel.cpp) is bound the same
# way: accessors, conditions, timestamps and quantities above keep their
# Python bodies under _py_* names, and the public names point at whichever
# path is live. NATIVE_OBJMODEL tells which. A native function hands any
# input it does not mirror exactly (a non-dict where a dict is expected, a
# datetime whose tzinfo is not timezone.utc) to the Python body of the same
# name, which is why the bodies are registered with set_fallbacks.
_native_objmodel = None
if os.environ.get("GPU_PROVISIONER_PURE_PYTHON") != "1":
    try:
        from .._native import _objmodel as _native_objmodel  # type: ignore
    except ImportError:
        _native_objmodel = None
NATIVE_OBJMODEL = _native_objmodel is not None

_impl = _native_objmodel if NATIVE_OBJMODEL else None
name_of = _impl.name_of if _impl else _py_name_of
namespace_of = _impl.namespace_of if _impl else _py_namespace_of
uid_of = _impl.uid_of if _impl else _py_uid_of
labels_of = _impl.labels_of if _impl else _py_labels_of
annotations_of = _impl.annotations_of if _impl else _py_annotations_of
finalizers_of = _impl.finalizers_of if _impl else _py_finalizers_of
has_finalizer = _impl.has_finalizer if _impl else _py_has_finalizer
is_deleting = _impl.is_deleting if _impl else _py_is_deleting
owner_references_of = _impl.owner_references_of if _impl else _py_owner_references_of
provider_id_of = _impl.provider_id_of if _impl else _py_provider_id_of
node_is_ready = _impl.node_is_ready if _impl else _py_node_is_ready
node_ready_condition = _impl.node_ready_condition if _impl else _py_node_ready_condition
get_condition = _impl.get_condition if _impl else _py_get_condition
condition_is = _impl.condition_is if _impl else _py_condition_is
condition_is_true = _impl.condition_is_true if _impl else _py_condition_is_true
set_condition = _impl.set_condition if _impl else _py_set_condition
fmt_time = _impl.fmt_time if _impl else _py_fmt_time
fmt_micro_time = _impl.fmt_micro_time if _impl else _py_fmt_micro_time
now_rfc3339 = _impl.now_rfc3339 if _impl else _py_now_rfc3339
uuid4_str = _impl.uuid4_str if _impl else _py_uuid4_str
Quantity = _NativeQuantity if _impl else _PyQuantity
if _impl:
    _impl.set_fallbacks(
        {k[len("_py_"):]: v for k, v in list(globals().items()) if k.startswith("_py_") and callable(v)}
    )


def group_version_kind(obj: dict) -> tuple:
    api = obj.get("apiVersion", "")
    if "/" in api:
        group, version = api.split("/", 1)
    else:
        group, version = "", api
    return group, version, obj.get("kind", "")
