"""Native object-model extension (native/objmodel.cpp) against the Python
bodies it replaces in kube/objects.py: accessors, conditions, timestamps,
uuid and Quantity.

Every test is differential: the native function and the retained _py_* body
get the same input and must give the same result (the same object where the
Python body returns a stored one) or raise the same exception type. Without
the built extension the native side is skipped by name; the fallback is then
what the rest of the suite already exercises."""
import copy
import itertools
import os
import re
import subprocess
import sys
import tracemalloc
import uuid
from datetime import datetime, timedelta, timezone
from fractions import Fraction

import pytest

from gpu_provisioner_amd.kube import informer as ki
from gpu_provisioner_amd.kube import objects as ko
from gpu_provisioner_amd.providers.instancetype.catalog import InstanceTypeProvider

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:
    from gpu_provisioner_amd._native import _objmodel as native
except ImportError:  # not built: only the fallback tests below can run
    native = None
else:
    # bind the Python bodies even when GPU_PROVISIONER_PURE_PYTHON=1 kept the
    # package from doing so: the native functions defer to them
    native.set_fallbacks(
        {k[4:]: v for k, v in vars(ko).items() if k.startswith("_py_") and callable(v)}
    )
    native.set_fallbacks({"object_key": ki._py_object_key})

needs_native = pytest.mark.skipif(native is None, reason="native _objmodel extension not built")
# the native-backed Quantity class calls the module the package bound, so it
# works only while the native path is live (built and not forced off)
needs_live = pytest.mark.skipif(not ko.NATIVE_OBJMODEL, reason="native object model not live")


class DictSub(dict):
    pass


class StrSub(str):
    pass


def cond(t, status="True", **extra):
    return {"type": t, "status": status, **extra}


FOUR = [cond("Launched"), cond("Registered", "False"), cond("Initialized", "Unknown"), cond("Ready")]


def corpus() -> list:
    """Objects with each field present, absent, None and empty; namespaced
    and cluster-scoped; 0, 1 and 4 conditions; and wrong-typed fields."""
    full_meta = {
        "name": "nc1", "namespace": "ns1", "uid": "u-1", "generation": 3,
        "labels": {"kaito.sh/workspace": "ws", "agentpool": "p1", "kubernetes.azure.com/agentpool": "p1"},
        "annotations": {"a": "1"}, "finalizers": ["karpenter.sh/termination", "x/y"],
        "deletionTimestamp": "2026-01-01T00:00:00Z",
        "ownerReferences": [{"uid": "o-1", "kind": "NodeClaim"}],
    }
    objs = [
        {},
        {"metadata": {}},
        {"metadata": dict(full_meta), "spec": {"providerID": "azure:///a", "nodeName": "n1"},
         "status": {"providerID": "azure:///b", "conditions": [dict(c) for c in FOUR]}},
        # cluster-scoped
        {"metadata": {"name": "node1", "labels": {"agentpool": "p1", "kubernetes.azure.com/agentpool": "p2"}},
         "spec": {"providerID": ""}, "status": {"conditions": [cond("Ready", "False")]}},
        {"metadata": {"name": "only-second-label", "labels": {"kubernetes.azure.com/agentpool": "p9"}}},
        {"metadata": {"namespace": "ns-without-name"}},
        # None and empty everywhere
        {"metadata": {k: None for k in full_meta}, "spec": {"providerID": None, "nodeName": None},
         "status": {"providerID": None, "conditions": None}},
        {"metadata": {"name": "", "namespace": "", "uid": "", "labels": {}, "annotations": {},
                      "finalizers": [], "deletionTimestamp": "", "ownerReferences": []},
         "spec": {}, "status": {"conditions": []}},
        {"metadata": {"name": "n"}, "status": {}},
        {"metadata": {"name": "n"}, "status": {"conditions": [cond("Ready")]}},
        {"metadata": {"name": "n"}, "status": {"conditions": [cond("Other"), {}, {"status": "True"}]}},
        {"metadata": {"name": "n"}, "status": {"conditions": [{"type": "Ready"}, cond("Ready")]}},
        {"metadata": {"name": "n"}, "status": {"conditions": [cond("Ready", None), cond("Launched", 1)]}},
        # wrong types: both sides must behave the same, including raising
        {"metadata": None},
        {"metadata": "text", "spec": None, "status": None},
        {"metadata": ["name"], "spec": 7, "status": 7},
        {"metadata": DictSub(name="sub", namespace="ns", labels=DictSub(agentpool="p")),
         "spec": DictSub(providerID="azure:///sub"), "status": DictSub(conditions=[cond("Ready")])},
        {"metadata": {"name": StrSub("strsub"), "namespace": StrSub("ns"), "labels": [("agentpool", "p")],
                      "finalizers": ("a", "b"), "deletionTimestamp": 0, "generation": "7"},
         "spec": {"providerID": 12, "nodeName": ["n"]},
         "status": {"providerID": StrSub("azure:///s"), "conditions": (cond("Ready"),)}},
        {"metadata": {"name": 5, "namespace": None, "labels": "ab", "finalizers": "abc"},
         "status": {"conditions": [cond("Ready"), "not-a-dict"]}},
        {"metadata": {"name": "n"}, "status": {"conditions": ["not-a-dict", cond("Ready")]}},
        {"metadata": {"name": "n"}, "status": {"conditions": [DictSub(type="Ready", status="True")]}},
        {"metadata": {"name": "n"}, "status": {"conditions": [cond(StrSub("Ready")), cond(7), cond(None)]}},
        {"metadata": {"name": "n"}, "status": {"conditions": {"type": "Ready"}}},
        DictSub(metadata={"name": "top-sub", "namespace": "ns"}),
        None,
        "text",
        [1],
    ]
    return objs


CORPUS = corpus()


def outcome(fn, *args, **kw):
    try:
        return ("ok", fn(*args, **kw))
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        return ("raised", type(e))


def stored_objects(tree, out=None) -> dict:
    """id -> object for everything reachable in a JSON tree"""
    out = {} if out is None else out
    out[id(tree)] = tree
    if isinstance(tree, dict):
        for v in tree.values():
            stored_objects(v, out)
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            stored_objects(v, out)
    return out


def assert_same(got, want, obj, label):
    assert got[0] == want[0], (label, obj, got, want)
    if got[0] == "raised":
        assert got[1] is want[1], (label, obj, got, want)
        return
    assert type(got[1]) is type(want[1]), (label, obj, got, want)
    assert got[1] == want[1], (label, obj, got, want)
    # where the Python body hands out an object stored in the tree, so does
    # the native one (the same object, not a copy)
    if id(want[1]) in stored_objects(obj) and isinstance(want[1], (dict, list, tuple, str)):
        assert got[1] is want[1], (label, obj)


UNARY = ["name_of", "namespace_of", "uid_of", "labels_of", "annotations_of", "finalizers_of",
         "is_deleting", "owner_references_of", "provider_id_of", "node_is_ready",
         "node_ready_condition"]
COND_TYPES = ["Launched", "Ready", "Registered", "Missing", "", None, 7, StrSub("Ready")]


@needs_native
def test_accessors_match_python_on_corpus():
    for obj in CORPUS:
        for name in UNARY:
            assert_same(outcome(getattr(native, name), obj),
                        outcome(getattr(ko, "_py_" + name), obj), obj, name)
        assert_same(outcome(native.object_key, obj), outcome(ki._py_object_key, obj), obj, "object_key")
        for fin in ["karpenter.sh/termination", "x/y", "a", "ab", "", None]:
            assert_same(outcome(native.has_finalizer, obj, fin),
                        outcome(ko._py_has_finalizer, obj, fin), obj, "has_finalizer")
        for t in COND_TYPES:
            assert_same(outcome(native.get_condition, obj, t),
                        outcome(ko._py_get_condition, obj, t), obj, "get_condition")
            assert_same(outcome(native.condition_is_true, obj, t),
                        outcome(ko._py_condition_is_true, obj, t), obj, "condition_is_true")
            for status in ["True", "False", "Unknown", None, 1]:
                assert_same(outcome(native.condition_is, obj, t, status),
                            outcome(ko._py_condition_is, obj, t, status), obj, "condition_is")


@needs_native
def test_accessor_defaults_are_fresh_containers():
    obj = {"metadata": {"labels": None, "finalizers": []}}
    a, b = native.labels_of(obj), native.labels_of(obj)
    assert a == {} and a is not b
    fins = native.finalizers_of(obj)
    assert fins == [] and fins is not obj["metadata"]["finalizers"]


@needs_native
def test_wrong_argument_counts_raise_like_python():
    obj = CORPUS[2]
    for name, args in [("has_finalizer", (obj,)), ("get_condition", (obj,)), ("condition_is", (obj, "Ready")),
                       ("condition_is_true", (obj, "Ready", "x")), ("set_condition", (obj, "Ready")),
                       ("set_condition", (obj, "A", "True", "r", "m", "extra"))]:
        assert outcome(getattr(native, name), *args) == outcome(getattr(ko, "_py_" + name), *args)
        assert outcome(getattr(native, name), *args) == ("raised", TypeError)
    assert outcome(native.set_condition, obj, "A", "True", nope=1) == ("raised", TypeError)
    assert outcome(native.set_condition, obj, "A", "True", "r", reason="twice") == ("raised", TypeError)


# ---------------------------------------------------------------------------
# set_condition
# ---------------------------------------------------------------------------

T0 = datetime(2026, 3, 4, 5, 6, 7, 123456, tzinfo=timezone.utc)
IST = timezone(timedelta(hours=5, minutes=30))

# (cond_type, status, reason, message, seconds after T0): add, same status
# with a new message, status flip, reason only, and a second type
SEQUENCE = [
    ("Launched", "Unknown", "", "", 0),
    ("Launched", "Unknown", "", "still waiting", 1),
    ("Launched", "True", "Launched", "still waiting", 2),
    ("Launched", "True", "Relaunched", "still waiting", 3),
    ("Launched", "True", "", "still waiting", 4),
    ("Registered", "False", "NodeNotFound", "no node yet", 5),
    ("Launched", "True", "Relaunched", "still waiting", 6),
    ("Registered", "True", "", "", 7),
]


def set_condition_starts() -> list:
    return [
        {},
        {"metadata": {"name": "a", "generation": 4}},
        {"metadata": {"name": "a"}, "status": {}},
        {"metadata": {"name": "a", "generation": 2}, "status": {"conditions": [dict(c) for c in FOUR]}},
        {"status": {"conditions": [{"type": "Launched"}, cond("Launched", "False", reason=None, message=None)]}},
    ]


@needs_native
def test_set_condition_sequence_matches_python():
    for start in set_condition_starts():
        a, b = ko._py_deep_copy(start), ko._py_deep_copy(start)
        for t, status, reason, message, dt in SEQUENCE:
            at = T0 + timedelta(seconds=dt)
            for style in range(3):
                if style == 0:
                    got = native.set_condition(a, t, status, reason, message, at=at)
                    want = ko._py_set_condition(b, t, status, reason, message, at=at)
                elif style == 1:
                    got = native.set_condition(a, t, status, reason=reason, message=message, at=at)
                    want = ko._py_set_condition(b, t, status, reason=reason, message=message, at=at)
                else:
                    got = native.set_condition(a, t, status, message=message, at=at)
                    want = ko._py_set_condition(b, t, status, message=message, at=at)
                assert got is want, (start, t, status, reason, message, style)
                assert a == b
                # key order of every condition dict, too
                assert [list(c) for c in a["status"]["conditions"]] == \
                       [list(c) for c in b["status"]["conditions"]]


@needs_native
def test_set_condition_other_datetimes_and_odd_shapes_match_python():
    ats = [T0.astimezone(IST), T0.replace(tzinfo=None), T0.astimezone(timezone(timedelta(0)))]
    odd = [o for o in CORPUS if isinstance(o, dict)] + [None, "text"]
    for obj in odd:
        for at in ats + [T0]:
            for args in [("Ready", "False", "Because", "msg"), ("New", "True", "", ""),
                         ("Ready", None, "", ""), (7, "True", "", ""), ("Ready", "True", None, 5)]:
                # copy.deepcopy: dict subclasses must not be shared by a and b
                a, b = copy.deepcopy(obj), copy.deepcopy(obj)
                got = outcome(native.set_condition, a, *args, at=at)
                want = outcome(ko._py_set_condition, b, *args, at=at)
                assert got == want, (obj, args, at)
                assert a == b, (obj, args, at)  # also after a partial write that raised


@needs_native
def test_set_condition_without_at_uses_the_clock_string():
    obj: dict = {}
    before = ko._py_fmt_time(ko.now())
    assert native.set_condition(obj, "Ready", "True") is True
    after = ko._py_fmt_time(ko.now())
    c = obj["status"]["conditions"][0]
    assert before <= c["lastTransitionTime"] <= after
    assert c == {"type": "Ready", "status": "True", "reason": "True", "message": "",
                 "lastTransitionTime": c["lastTransitionTime"], "observedGeneration": 0}
    assert native.set_condition(obj, "Ready", "True") is False


# ---------------------------------------------------------------------------
# time, uuid
# ---------------------------------------------------------------------------


class DatetimeSub(datetime):
    pass


@needs_native
def test_fmt_time_matches_python():
    times = [
        T0, T0.astimezone(IST), T0.replace(tzinfo=None),
        datetime(1, 1, 1, tzinfo=timezone.utc), datetime(9999, 12, 31, 23, 59, 59, 999999, tzinfo=timezone.utc),
        datetime(987, 6, 5, 4, 3, 2, 1, tzinfo=timezone.utc),
        T0.astimezone(timezone(timedelta(0))),  # UTC offset, but not the timezone.utc object
        DatetimeSub(2026, 1, 2, 3, 4, 5, 6, tzinfo=timezone.utc),
        "2026-01-01", None,
    ]
    for t in times:
        assert outcome(native.fmt_time, t) == outcome(ko._py_fmt_time, t), t
        assert outcome(native.fmt_micro_time, t) == outcome(ko._py_fmt_micro_time, t), t
    assert native.fmt_time(T0) == "2026-03-04T05:06:07Z"
    assert native.fmt_micro_time(T0) == "2026-03-04T05:06:07.123456Z"
    assert native.fmt_time(T0.astimezone(IST)) == "2026-03-04T05:06:07Z"


@pytest.mark.parametrize("impl", ["native", "python"])
def test_now_rfc3339(impl):
    if impl == "native" and native is None:
        pytest.skip("native _objmodel extension not built")
    fn = native.now_rfc3339 if impl == "native" else ko._py_now_rfc3339
    before = ko._py_fmt_time(ko.now())
    got = fn()
    after = ko._py_fmt_time(ko.now())
    assert re.match(r"^\d{4}-\d\d-\d\dT\d\d:\d\d:\d\dZ$", got)
    assert before <= got <= after
    # two calls inside one second: equal strings. Up to three attempts, as a
    # pair of calls can straddle a second boundary (it cannot three times).
    for _ in range(3):
        t0 = ko.now()
        a, b = fn(), fn()
        if ko.now().replace(microsecond=0) == t0.replace(microsecond=0):
            assert a == b == ko._py_fmt_time(t0)
            if impl == "native":
                assert a is b  # the cached object
            break
    else:
        pytest.fail("three pairs of calls each straddled a second boundary")


@pytest.mark.parametrize("impl", ["native", "python"])
def test_uuid4_str(impl):
    if impl == "native" and native is None:
        pytest.skip("native _objmodel extension not built")
    fn = native.uuid4_str if impl == "native" else ko._py_uuid4_str
    draws = [fn() for _ in range(1000)]
    assert len(set(draws)) == 1000
    for s in draws:
        assert re.match(r"^[0-9a-f]{8}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{4}-[0-9a-f]{12}$", s)
        u = uuid.UUID(s)
        assert str(u) == s and u.version == 4 and u.variant == uuid.RFC_4122


# ---------------------------------------------------------------------------
# Quantity
# ---------------------------------------------------------------------------

NUMBERS = ["0", "1", "8", "007", "100", "2036", "0.5", ".5", "1.5", "0.001", "0.0001", "1.0005",
           "123456789", "999999999999999999", "1234567890123456789", "0.1234567890123456789",
           "12345678901234567890123", "0.000000000000000001"]
STRINGS = ([f"{sign}{n}{suf}" for n in NUMBERS for suf in ko._SUFFIX for sign in ("", "-")]
           + ["+8", "+1.5Gi", "500m", "1.5Gi", "2036Gi", "100Mi", "240m", "-0", "-0m", "16Ei", "9Ei"])
INVALID = ["", "m", "Gi", "8Zi", "8 Gi", " 8", "8 ", "1e3", "1e", "5.", "5.Gi", "--5", "+-5", "1..2",
           "1.2.3", "8gi", "8KI", "8mi", "٣", "8\u0660", "1_000", "0x10", "8G i", "8\x00", "nan", "inf"]
OTHER_INPUTS = [0, 1, -7, 2**70, True, 0.5, 0.1, 1e18, -2.25, Fraction(1, 3), Fraction(5, 1),
                Fraction(-3, 1000), Fraction(7, 2), Fraction(2**80, 3), StrSub("1.5Gi"), "8\n", None, [1]]


def same_quantity(q, ref):
    assert type(q.raw) is type(ref.raw) and q.raw == ref.raw
    assert str(q) == str(ref) and repr(q) == repr(ref)
    assert type(q.value) is Fraction and q.value == ref.value
    assert hash(q) == hash(ref)
    assert q.is_zero() == ref.is_zero()


@needs_live
def test_quantity_construction_matches_python():
    for raw in STRINGS + OTHER_INPUTS:
        want = outcome(ko._PyQuantity, raw)
        got = outcome(ko._NativeQuantity, raw)
        assert got[0] == want[0], raw
        if want[0] == "raised":
            assert got[1] is want[1], raw
        else:
            same_quantity(got[1], want[1])
            same_quantity(ko._NativeQuantity(got[1]), want[1])
    for raw in INVALID:
        with pytest.raises(ValueError) as py_err:
            ko._PyQuantity(raw)
        with pytest.raises(ValueError) as native_err:
            ko._NativeQuantity(raw)
        assert str(native_err.value) == str(py_err.value), raw
    assert hash(ko._NativeQuantity("8")) == hash(8) == hash(ko._NativeQuantity("8000m"))
    assert hash(ko._NativeQuantity("2Ki")) == hash(2048)


@needs_live
def test_quantity_pairs_match_python():
    grid = ["0", "8", "-8", "8000m", "240m", "-240m", "0.5", "1.5Gi", "2036Gi", "100Mi", "1Ei", "9Ei",
            "16Ei", "999999999999999999E", "0.001m", "0.0001", "1.0005k", "999999999999999999",
            "0.000000000000000001", "12345678901234567890123Ki", 7, 0.1, Fraction(1, 3), Fraction(2**80, 3)]
    for ra, rb in itertools.product(grid, repeat=2):
        a, b = ko._NativeQuantity(ra), ko._NativeQuantity(rb)
        pa, pb = ko._PyQuantity(ra), ko._PyQuantity(rb)
        assert (a == b) is (pa == pb), (ra, rb)
        assert (a != b) is (pa != pb), (ra, rb)
        assert (a < b) is (pa < pb), (ra, rb)
        assert (a <= b) is (pa <= pb), (ra, rb)
        assert (a > b) is (pa > pb), (ra, rb)
        assert (a >= b) is (pa >= pb), (ra, rb)
        assert (hash(a) == hash(b)) is (hash(pa) == hash(pb)), (ra, rb)
        same_quantity(a + b, pa + pb)
        same_quantity(a - b, pa - pb)
    assert ko._NativeQuantity("8") != 8 and ko._NativeQuantity("8") != "8"
    assert str(ko._NativeQuantity("2036Gi") - ko._NativeQuantity("100Mi")) == "2186033496064"
    assert str(ko._NativeQuantity("96") - ko._NativeQuantity("240m")) == "95760m"
    assert str(ko._NativeQuantity("1") - ko._NativeQuantity("0.0001")) == "0.9999"


@needs_native
def test_native_quantity_helpers_reject_what_they_do_not_cover():
    assert native.qty_parse("1234567890123456789") is None  # 19 digits
    assert native.qty_parse("16Ei") is None  # beyond 64 bits
    assert native.qty_parse(StrSub("8")) is None and native.qty_parse(8) is None
    assert native.qty_parse("1.5Gi") == (1610612736, 1)
    assert native.qty_parse("-500m") == (-1, 2)
    assert native.qty_addsub(2**63, 1, 1, 1, False) is None
    assert native.qty_addsub(2**62, 1, 2**62, 1, False) is None
    assert native.qty_addsub(1, 3, 1, 6, False) == (1, 2, "500m")
    assert native.qty_fmt(2**200, 1) == str(2**200)
    assert native.qty_fmt(1, 3) == str(1 / 3)
    with pytest.raises(TypeError):
        native.qty_fmt("1", 1)


def test_allocatable_matches_python_for_every_catalog_sku():
    """Runs on whichever Quantity is live; the reference is the Python class."""
    types = InstanceTypeProvider().list()
    assert len(types) >= 1
    for it in types:
        want = {}
        for res, cap in it.capacity.items():
            ovh = it.overhead.get(res)
            want[res] = str(ko._PyQuantity(cap) - ko._PyQuantity(ovh)) if ovh else str(cap)
        assert it.allocatable() == want, it.name
        assert list(it.allocatable()) == list(want)


# ---------------------------------------------------------------------------
# leaks
# ---------------------------------------------------------------------------


@needs_native
def test_no_reference_or_memory_leak():
    name, fin, ctype = "name-%d" % os.getpid(), "fin-%d" % os.getpid(), "Type-%d" % os.getpid()
    conds = [cond("Launched"), cond(ctype, "False", reason="r", message="m")]
    labels = {"agentpool": name}
    obj = {"metadata": {"name": name, "namespace": name, "uid": name, "labels": labels,
                        "finalizers": [fin], "generation": 123456789},
           "spec": {"providerID": name}, "status": {"conditions": conds}}
    bare: dict = {"metadata": {"labels": None}}
    odd = {"metadata": None}
    at = T0
    state = {"n": 0}

    def flip():
        state["n"] += 1
        native.set_condition(obj, ctype, "True" if state["n"] % 2 else "False", "r%d" % (state["n"] % 3), at=at)

    def odd_raises():
        try:
            native.name_of(odd)
        except AttributeError:
            pass

    calls = [
        lambda: native.name_of(obj), lambda: native.namespace_of(obj), lambda: native.uid_of(bare),
        lambda: native.labels_of(obj), lambda: native.labels_of(bare), lambda: native.annotations_of(obj),
        lambda: native.finalizers_of(obj), lambda: native.finalizers_of(bare),
        lambda: native.has_finalizer(obj, fin), lambda: native.is_deleting(obj),
        lambda: native.owner_references_of(obj), lambda: native.provider_id_of(obj),
        lambda: native.object_key(obj), lambda: native.get_condition(obj, ctype),
        lambda: native.condition_is(obj, ctype, "True"), lambda: native.condition_is_true(obj, ctype),
        lambda: native.node_is_ready(obj), lambda: native.node_ready_condition(obj),
        lambda: native.get_condition(obj, 7),  # deferred to the Python body
        odd_raises, flip,
        lambda: native.set_condition(obj, ctype, "True", "same", "same", at=at),
        lambda: native.set_condition({}, ctype, "True"),
        lambda: native.fmt_time(at), lambda: native.fmt_micro_time(at),
        lambda: native.fmt_time(at.astimezone(IST)),
        native.now_rfc3339, native.uuid4_str,
        lambda: native.qty_parse("1.5Gi"), lambda: native.qty_parse("bad"),
        lambda: native.qty_fmt(1, 3), lambda: native.qty_addsub(1, 3, 1, 6, True),
    ]
    if ko.NATIVE_OBJMODEL:
        calls.append(lambda: str(ko._NativeQuantity("2036Gi") - ko._NativeQuantity("100Mi")))
    # objects of this test only: None and the bools are also touched by the
    # Python bodies that deferred calls run, so their counts are not steady
    watched = (name, fin, ctype, conds, labels, obj, at)

    def refs():
        return [sys.getrefcount(o) for o in watched]

    for call in calls:
        call()  # first-use allocations happen here
        call()
        tracemalloc.start()
        before_refs, before_mem = refs(), tracemalloc.get_traced_memory()[0]
        for _ in range(5000):
            call()
        after_mem = tracemalloc.get_traced_memory()[0]
        tracemalloc.stop()
        assert refs() == before_refs, calls.index(call)
        assert after_mem - before_mem < 64 << 10, calls.index(call)


# ---------------------------------------------------------------------------
# fallback
# ---------------------------------------------------------------------------

FALLBACK_SCRIPT = """
import asyncio, sys
sys.path.insert(0, %r)
from gpu_provisioner_amd.kube import objects as ko, informer as ki
from gpu_provisioner_amd.apis import v1 as karpv1
from gpu_provisioner_amd.fake.harness import Harness
print("NATIVE_OBJMODEL", ko.NATIVE_OBJMODEL)
assert ko.name_of is ko._py_name_of and ko.set_condition is ko._py_set_condition
assert ko.fmt_time is ko._py_fmt_time and ko.now_rfc3339 is ko._py_now_rfc3339
assert ko.uuid4_str is ko._py_uuid4_str and ko.Quantity is ko._PyQuantity
assert ki.object_key is ki._py_object_key and ki._index_store is ki._py_index_store
assert ki.field_index is ki._py_field_index

async def cycle():
    h = Harness(node_wait_interval=0.005).add_all_controllers(
        lifecycle_workers=8, termination_requeue=0.01, drain_requeue=0.01,
        instance_poll=0.01, gc_interval=30.0)
    await h.start()
    try:
        await h.kube.create(h.make_nodeclaim("fb1"))
        done = await h.wait_initialized("fb1", timeout=30.0)
        assert karpv1.is_initialized(done)
        await h.kube.delete(karpv1.API_VERSION, karpv1.KIND_NODECLAIM, "fb1")
        await h.wait_gone(karpv1.API_VERSION, karpv1.KIND_NODECLAIM, "fb1", timeout=30.0)
    finally:
        await h.stop()

asyncio.run(cycle())
print("CYCLE OK")
"""


def test_pure_python_env_forces_fallback():
    env = dict(os.environ, GPU_PROVISIONER_PURE_PYTHON="1")
    proc = subprocess.run(
        [sys.executable, "-c", FALLBACK_SCRIPT % ROOT],
        env=env, capture_output=True, text=True, timeout=120,
    )
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "NATIVE_OBJMODEL False" in proc.stdout
    assert "CYCLE OK" in proc.stdout


def test_native_flag_reports_live_path():
    forced = os.environ.get("GPU_PROVISIONER_PURE_PYTHON") == "1"
    assert ko.NATIVE_OBJMODEL == (native is not None and not forced)
    if ko.NATIVE_OBJMODEL:
        assert ko.name_of is native.name_of and ko.set_condition is native.set_condition
        assert ko.now_rfc3339 is native.now_rfc3339 and ko.uuid4_str is native.uuid4_str
        assert ko.Quantity is ko._NativeQuantity
        assert ki.object_key is native.object_key and ki._index_store is native.index_store
    else:
        assert ko.name_of is ko._py_name_of and ko.Quantity is ko._PyQuantity
        assert ki._index_store is ki._py_index_store
