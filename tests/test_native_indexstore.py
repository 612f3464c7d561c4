"""Native informer index store (native/objmodel.cpp: field_index,
index_store) against the Python bodies in kube/informer.py.

A random event sequence is replayed through both stores; after every event
the cache and every index dict must be equal, with no empty bucket left.
Without the built extension the native side is skipped by name."""
import os
import random
import sys
import tracemalloc
from collections import defaultdict

import pytest

from gpu_provisioner_amd.apis import v1 as karpv1
from gpu_provisioner_amd.kube import informer as ki
from gpu_provisioner_amd.kube.client import ADDED, DELETED, MODIFIED

from test_native_objmodel import CORPUS, assert_same, native, needs_native, outcome

PROVIDER_ID = ("spec", "providerID")
STATUS_PROVIDER_ID = ("status", "providerID")
NODE_NAME = ("spec", "nodeName")
AGENTPOOL = (("metadata", "labels", karpv1.AGENTPOOL_LABEL_KEY),
             ("metadata", "labels", karpv1.AZURE_AGENTPOOL_LABEL_KEY))


def native_field_index(*paths):
    return native.field_index(ki._py_field_index(*paths), *paths)


# the lambdas field_index replaced at the registration sites
def agentpool_lambda(o):
    return [
        v
        for v in (
            (o.get("metadata", {}).get("labels") or {}).get(karpv1.AGENTPOOL_LABEL_KEY),
            (o.get("metadata", {}).get("labels") or {}).get(karpv1.AZURE_AGENTPOOL_LABEL_KEY),
        )
        if v
    ] or None


REPLACED = [
    ((PROVIDER_ID,), lambda o: o.get("spec", {}).get("providerID") or None),
    ((STATUS_PROVIDER_ID,), lambda o: o.get("status", {}).get("providerID") or None),
    ((NODE_NAME,), lambda o: o.get("spec", {}).get("nodeName") or None),
    (AGENTPOOL, agentpool_lambda),
]


def as_index_values(res):
    """What the informer makes of an index function's result: a single
    string is one value (the replaced single-path lambdas return the bare
    string, field_index returns the list add_index documents)."""
    if res[0] == "ok" and isinstance(res[1], str):
        return ("ok", [res[1]])
    return res


@pytest.mark.parametrize("impl", ["native", "python"])
def test_field_index_equals_the_lambda_it_replaces(impl):
    if impl == "native" and native is None:
        pytest.skip("native _objmodel extension not built")
    make = native_field_index if impl == "native" else ki._py_field_index
    extra = [
        {"metadata": {"labels": {karpv1.AGENTPOOL_LABEL_KEY: "same", karpv1.AZURE_AGENTPOOL_LABEL_KEY: "same"}}},
        {"metadata": {"labels": {karpv1.AGENTPOOL_LABEL_KEY: "", karpv1.AZURE_AGENTPOOL_LABEL_KEY: "b"}}},
        {"metadata": {"labels": {karpv1.AGENTPOOL_LABEL_KEY: "a", karpv1.AZURE_AGENTPOOL_LABEL_KEY: "b"}}},
        {"metadata": {"labels": {karpv1.AGENTPOOL_LABEL_KEY: 5}}},
        {"metadata": {"labels": None}}, {"metadata": {"labels": ""}}, {"metadata": {"labels": 0}},
        {"spec": {"providerID": "azure:///x", "nodeName": "n"}, "status": {"providerID": "azure:///y"}},
    ]
    for paths, lam in REPLACED:
        fn = make(*paths)
        for obj in CORPUS + extra:
            got, want = outcome(fn, obj), as_index_values(outcome(lam, obj))
            assert_same(got, want, obj, paths)
            if got[0] == "ok" and isinstance(got[1], list) and len(paths) > 1:
                assert all(got[1])
    assert make(AGENTPOOL[0], AGENTPOOL[1])(extra[2]) == ["a", "b"]  # path order
    assert make(("kind",))({"kind": "Node"}) == ["Node"]


@needs_native
def test_field_index_rejects_bad_paths():
    for paths in [(), ((),), (("a", 1),), ("ab", 5)]:
        with pytest.raises(TypeError):
            native.field_index(lambda o: None, *paths)
    with pytest.raises(TypeError):
        native.field_index(None, ("a",))


# ---------------------------------------------------------------------------
# replay
# ---------------------------------------------------------------------------


def make_indexes(native_side: bool) -> dict:
    fi = native_field_index if native_side else ki._py_field_index
    return {
        "providerID": (fi(PROVIDER_ID), defaultdict(set)),
        "agentpool": (fi(*AGENTPOOL), defaultdict(set)),
        # arbitrary Python index functions keep working beside native ones:
        # one returning a bare string or None, one returning a tuple
        "zone": (lambda o: (o.get("metadata", {}).get("labels") or {}).get("zone"), defaultdict(set)),
        "owners": (lambda o: tuple(r["uid"] for r in o.get("metadata", {}).get("ownerReferences") or ()),
                   defaultdict(set)),
    }


def random_revision(rng: random.Random, name: str, namespace: str) -> dict:
    meta: dict = {"name": name}
    if namespace:
        meta["namespace"] = namespace
    labels = {}
    if rng.random() < 0.7:
        labels[karpv1.AGENTPOOL_LABEL_KEY] = rng.choice(["p1", "p2", "p3", ""])
    if rng.random() < 0.7:
        # often the same value under both label keys
        labels[karpv1.AZURE_AGENTPOOL_LABEL_KEY] = rng.choice(
            [labels.get(karpv1.AGENTPOOL_LABEL_KEY, "p1"), "p2", "p4"])
    if rng.random() < 0.5:
        labels["zone"] = rng.choice(["z1", "z2"])
    if labels or rng.random() < 0.5:
        meta["labels"] = labels if rng.random() < 0.9 else None
    if rng.random() < 0.4:
        meta["ownerReferences"] = [{"uid": rng.choice(["o1", "o2", "o3"])} for _ in range(rng.randrange(3))]
    obj: dict = {"metadata": meta}
    roll = rng.random()
    if roll < 0.6:  # write-once in real use: mostly the same value per name
        obj["spec"] = {"providerID": "azure:///%s" % name if rng.random() < 0.8 else rng.choice(["azure:///shared", "", None])}
    elif roll < 0.8:
        obj["spec"] = {}
    return obj


def events(seed: int, steps: int):
    rng = random.Random(seed)
    live: dict = {}
    names = [("n%d" % i, rng.choice(["", "", "ns1"])) for i in range(12)]
    for _ in range(steps):
        name, ns = rng.choice(names)
        key = f"{ns}/{name}" if ns else name
        roll = rng.random()
        if key not in live:
            if roll < 0.1:  # DELETED for an object the cache never saw
                yield DELETED, key, random_revision(rng, name, ns)
                continue
            live[key] = random_revision(rng, name, ns)
            yield ADDED, key, live[key]
        elif roll < 0.2:
            yield DELETED, key, live.pop(key)
        elif roll < 0.3:
            yield MODIFIED, key, live[key]  # resync: the same revision again
        else:
            live[key] = random_revision(rng, name, ns)
            yield MODIFIED, key, live[key]


def apply(store, event, key, obj, indexes, cache):
    if event == DELETED:
        store(key, cache.get(key) or obj, None, indexes, cache)
    else:
        store(key, cache.get(key), obj, indexes, cache)


def snapshot(indexes: dict) -> dict:
    return {name: {v: set(keys) for v, keys in idx.items()} for name, (_, idx) in indexes.items()}


@pytest.mark.parametrize("seed", [1, 2, 3])
@needs_native
def test_replay_matches_python_store_after_every_event(seed):
    nat_idx, py_idx = make_indexes(True), make_indexes(False)
    nat_cache: dict = {}
    py_cache: dict = {}
    seen = {ADDED: 0, MODIFIED: 0, DELETED: 0}
    for event, key, obj in events(seed, 1500):
        seen[event] += 1
        assert native.object_key(obj) == ki._py_object_key(obj) == key
        apply(native.index_store, event, key, obj, nat_idx, nat_cache)
        apply(ki._py_index_store, event, key, obj, py_idx, py_cache)
        assert nat_cache == py_cache
        assert all(nat_cache[k] is py_cache[k] for k in py_cache)
        got, want = snapshot(nat_idx), snapshot(py_idx)
        assert got == want
        for name, buckets in got.items():
            assert all(buckets.values()), "empty bucket left in %s" % name
    assert min(seen.values()) > 50
    # what is indexed is exactly what a fresh pass over the cache would index
    fresh = make_indexes(False)
    for key, obj in py_cache.items():
        ki._py_index_store(key, None, obj, fresh, {})
    assert snapshot(nat_idx) == snapshot(fresh)


@pytest.mark.parametrize("impl", ["native", "python"])
def test_unchanged_index_value_leaves_the_bucket_alone_or_equal(impl):
    if impl == "native" and native is None:
        pytest.skip("native _objmodel extension not built")
    store = native.index_store if impl == "native" else ki._py_index_store
    indexes = make_indexes(impl == "native")
    cache: dict = {}
    a1 = {"metadata": {"name": "a"}, "spec": {"providerID": "azure:///a"}}
    a2 = {"metadata": {"name": "a", "labels": {"zone": "z1"}}, "spec": {"providerID": "azure:///a"}}
    store("a", None, a1, indexes, cache)
    bucket = indexes["providerID"][1]["azure:///a"]
    store("a", a1, a2, indexes, cache)
    assert cache == {"a": a2} and indexes["providerID"][1] == {"azure:///a": {"a"}}
    assert indexes["zone"][1] == {"z1": {"a"}}
    if impl == "native":
        assert indexes["providerID"][1]["azure:///a"] is bucket  # not rebuilt
    store("a", a2, None, indexes, cache)
    assert cache == {} and all(not idx for _, idx in indexes.values())


@needs_native
def test_index_store_errors():
    cache: dict = {}
    with pytest.raises(TypeError):
        native.index_store("k", None, {}, {}, [])
    with pytest.raises(TypeError):
        native.index_store("k", None, {}, {"bad": "entry"}, cache)
    with pytest.raises(TypeError):
        native.index_store("k", None, {"a": 1}, {"i": (lambda o: "v", {"v": ["not a set"]})}, cache)

    def boom(o):
        raise RuntimeError("index function failed")

    indexes = {"ok": (native_field_index(PROVIDER_ID), defaultdict(set)), "boom": (boom, defaultdict(set))}
    with pytest.raises(RuntimeError):
        native.index_store("k", None, {"spec": {"providerID": "p"}}, indexes, cache)
    # every index function runs before the first write: nothing was touched
    assert cache == {} and not indexes["ok"][1]


@needs_native
def test_informer_uses_native_store_when_live():
    import asyncio

    from gpu_provisioner_amd.fake.apiserver import InMemoryAPIServer, InMemoryClient
    from gpu_provisioner_amd.kube import objects as ko
    from gpu_provisioner_amd.kube.informer import Informer

    if not ko.NATIVE_OBJMODEL:
        pytest.skip("native path forced off")

    async def run():
        api = InMemoryClient(InMemoryAPIServer())
        inf = Informer(api, "v1", "Node")
        inf.add_index("providerID", ki.field_index(PROVIDER_ID))
        inf.add_index("first-letter", lambda o: ko.name_of(o)[:1])
        inf.start()
        await inf.wait_for_sync()
        node = {"apiVersion": "v1", "kind": "Node", "metadata": {"name": "n1"}, "spec": {"providerID": "azure:///n1"}}
        await api.create(node)
        await inf.wait_until(lambda e, o: o, name="n1", timeout=5.0)
        assert [ko.name_of(o) for o in inf.by_index("providerID", "azure:///n1")] == ["n1"]
        assert [ko.name_of(o) for o in inf.by_index("first-letter", "n")] == ["n1"]
        await api.delete("v1", "Node", "n1")
        await inf.wait_until(lambda e, o: True if e in (DELETED, "ABSENT") else None, name="n1", timeout=5.0)
        assert inf.by_index("providerID", "azure:///n1") == []
        assert not inf._indexes["providerID"][1] and not inf._indexes["first-letter"][1]
        await inf.stop()

    assert type(ki.field_index(PROVIDER_ID)).__name__ == "FieldIndex"
    asyncio.run(run())


# ---------------------------------------------------------------------------
# leaks
# ---------------------------------------------------------------------------


@needs_native
def test_no_reference_or_memory_leak():
    key, pid, pool = "key-%d" % os.getpid(), "azure:///%d" % os.getpid(), "pool-%d" % os.getpid()
    rev1 = {"metadata": {"name": key, "labels": {karpv1.AGENTPOOL_LABEL_KEY: pool}}, "spec": {"providerID": pid}}
    rev2 = {"metadata": {"name": key, "labels": {karpv1.AZURE_AGENTPOOL_LABEL_KEY: pool, "zone": "z"}},
            "spec": {"providerID": pid}}
    rev3 = {"metadata": {"name": key}}
    odd = {"metadata": {"labels": {karpv1.AGENTPOOL_LABEL_KEY: 5}}, "spec": None}
    indexes = make_indexes(True)
    cache: dict = {}
    fi = native_field_index(*AGENTPOOL)

    def churn():
        native.index_store(key, None, rev1, indexes, cache)
        native.index_store(key, rev1, rev2, indexes, cache)
        native.index_store(key, rev2, rev2, indexes, cache)
        native.index_store(key, rev2, rev3, indexes, cache)
        native.index_store(key, rev3, None, indexes, cache)

    def odd_call():
        assert fi(odd) == [5]  # deferred to the Python indexer
        try:
            native_field_index(PROVIDER_ID)(odd)
        except AttributeError:
            pass

    calls = [churn, lambda: fi(rev1), lambda: fi(rev3), odd_call,
             lambda: native_field_index(PROVIDER_ID, NODE_NAME)]
    watched = (key, pid, pool, rev1, rev2, rev3, indexes, cache)

    def refs():
        return [sys.getrefcount(o) for o in watched]

    for call in calls:
        call()
        call()
        tracemalloc.start()
        before_refs, before_mem = refs(), tracemalloc.get_traced_memory()[0]
        for _ in range(3000):
            call()
        after_mem = tracemalloc.get_traced_memory()[0]
        tracemalloc.stop()
        assert refs() == before_refs, calls.index(call)
        assert after_mem - before_mem < 64 << 10, calls.index(call)
    assert cache == {} and all(not idx for _, idx in indexes.values())
