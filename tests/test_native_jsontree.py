"""Native JSON-tree extension (native/jsontree.cpp) against the pure-Python
functions it replaces: deep_copy, json_merge_patch, merge_patch_owned.

Every equivalence test compares the native function with the retained Python
body. Without the built extension the native side is skipped by name (the
fallback is then what the rest of the suite already exercises)."""
import os
import random
import subprocess
import sys
import tracemalloc

import pytest

from gpu_provisioner_amd.kube import client as kc
from gpu_provisioner_amd.kube import objects as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:
    from gpu_provisioner_amd._native import _jsontree as native
except ImportError:  # not built: only the fallback tests below can run
    native = None

needs_native = pytest.mark.skipif(native is None, reason="native _jsontree extension not built")


class DictSub(dict):
    pass


class ListSub(list):
    pass


def random_tree(rng: random.Random, depth: int):
    """JSON tree of depth <= `depth` with every leaf kind, plus dict/list
    subclass instances and tuples as inner values (shared, never copied)."""
    kind = rng.random()
    if depth == 0 or kind < 0.25:
        return rng.choice(
            [None, True, False, rng.randrange(-5, 10**12), rng.random() * 1e6,
             "s%d" % rng.randrange(1000), "", (1, [2], {"t": 3}),
             DictSub(a=[1]), ListSub([{"b": 2}])]
        )
    if kind < 0.65:
        return {
            "k%d" % rng.randrange(12): random_tree(rng, depth - 1)
            for _ in range(rng.randrange(0, 6))
        }
    return [random_tree(rng, depth - 1) for _ in range(rng.randrange(0, 5))]


EDGE_TREES = [
    {}, [], 7, "x", None, True, 1.5, (1, 2), [[], [[]], [[1], [2, [3]]]],
    {"a": DictSub(x=[1]), "b": ListSub([1, {}]), "c": (1, [2])},
    [DictSub(), ListSub(), {"z": None, "y": False, "x": 0, "w": 0.0, "v": ""}],
    {"b": 1, "a": 2, "c": {"z": 1, "a": 2}},
]


def corpus() -> list:
    rng = random.Random(20260)
    return EDGE_TREES + [random_tree(rng, rng.randrange(1, 7)) for _ in range(500)]


CORPUS = corpus()


def assert_copied(src, dst):
    """dst is a deep_copy of src: exact dict/list fresh, all else shared."""
    if type(src) is dict:
        assert type(dst) is dict and dst is not src
        assert list(dst) == list(src)  # key order
        for k in src:
            assert_copied(src[k], dst[k])
    elif type(src) is list:
        assert type(dst) is list and dst is not src and len(dst) == len(src)
        for a, b in zip(src, dst):
            assert_copied(a, b)
    else:
        assert dst is src


# ---------------------------------------------------------------------------
# copy
# ---------------------------------------------------------------------------


@needs_native
def test_deep_copy_matches_python_on_corpus():
    for tree in CORPUS:
        got, want = native.deep_copy(tree), ko._py_deep_copy(tree)
        assert got == want == tree
        assert_copied(tree, got)
        assert_copied(tree, want)


@pytest.mark.parametrize("impl", ["native", "python"])
def test_deep_copy_too_deep_or_cyclic_raises_recursion_error(impl):
    if impl == "native" and native is None:
        pytest.skip("native _jsontree extension not built")
    fn = native.deep_copy if impl == "native" else ko._py_deep_copy
    deep: list = []
    for _ in range(100_000):
        deep = [deep]
    with pytest.raises(RecursionError):
        fn(deep)
    cyc: dict = {"a": 1}
    cyc["self"] = cyc
    with pytest.raises(RecursionError):
        fn(cyc)
    cyc_list: list = [1]
    cyc_list.append({"l": cyc_list})
    with pytest.raises(RecursionError):
        fn(cyc_list)
    # unlink the deep chain iteratively so its teardown does not recurse
    while deep:
        deep = deep.pop()


# ---------------------------------------------------------------------------
# merge patch
# ---------------------------------------------------------------------------

# RFC 7386 appendix A: (target, patch, result)
RFC_CASES = [
    ({"a": "b"}, {"a": "c"}, {"a": "c"}),
    ({"a": "b"}, {"b": "c"}, {"a": "b", "b": "c"}),
    ({"a": "b"}, {"a": None}, {}),
    ({"a": "b", "b": "c"}, {"a": None}, {"b": "c"}),
    ({"a": ["b"]}, {"a": "c"}, {"a": "c"}),
    ({"a": "c"}, {"a": ["b"]}, {"a": ["b"]}),
    ({"a": {"b": "c"}}, {"a": {"b": "d", "c": None}}, {"a": {"b": "d"}}),
    ({"a": [{"b": "c"}]}, {"a": [1]}, {"a": [1]}),
    (["a", "b"], ["c", "d"], ["c", "d"]),
    ({"a": "b"}, ["c"], ["c"]),
    ({"a": "foo"}, None, None),
    ({"a": "foo"}, "bar", "bar"),
    ({"e": None}, {"a": 1}, {"e": None, "a": 1}),
    ([1, 2], {"a": "b", "c": None}, {"a": "b"}),
    ({}, {"a": {"bb": {"ccc": None}}}, {"a": {"bb": {}}}),
]


def stored_nodeclaim() -> dict:
    return {
        "apiVersion": "karpenter.sh/v1",
        "kind": "NodeClaim",
        "metadata": {
            "name": "nc1",
            "uid": "u-1",
            "resourceVersion": "41",
            "generation": 1,
            "labels": {"kaito.sh/workspace": "ws"},
            "annotations": {"a": "1"},
            "finalizers": ["karpenter.sh/termination"],
        },
        "spec": {
            "requirements": [{"key": "node.kubernetes.io/instance-type", "operator": "In",
                              "values": ["Standard_ND128isr_MI355X_v6"]}],
            "resources": {"requests": {"amd.com/gpu": "8"}},
            "nodeClassRef": {"group": "kaito.sh", "kind": "KaitoNodeClass", "name": "default"},
        },
        "status": {
            "providerID": "azure:///x",
            "conditions": [{"type": "Launched", "status": "True", "reason": "Launched",
                            "lastTransitionTime": "2026-01-01T00:00:00Z"}],
        },
    }


def project_patches() -> list:
    return [
        # status patch carrying a conditions list
        {"status": {"nodeName": "n1", "conditions": [
            {"type": "Launched", "status": "True"}, {"type": "Registered", "status": "True"}]}},
        # metadata finalizer removal
        {"metadata": {"finalizers": []}},
        {"metadata": {"finalizers": None}},
        # null deleting a key, at the top and nested
        {"status": None},
        {"metadata": {"annotations": {"a": None, "b": "2"}}},
        {"metadata": {"labels": {"x": "y"}}, "spec": {"resources": {"requests": {"cpu": "1"}}}},
        {},
        {"metadata": None},
        {"new": {"deep": {"list": [{"a": [1, 2]}], "gone": None}}},
        {"spec": "scalar"},
    ]


def merge_inputs() -> list:
    rng = random.Random(7386)
    cases = [(t, p) for t, p, _ in RFC_CASES]
    cases += [(stored_nodeclaim(), p) for p in project_patches()]
    for _ in range(300):
        cases.append((random_tree(rng, rng.randrange(0, 5)), random_tree(rng, rng.randrange(0, 5))))
    cases.append((DictSub(a={"b": 1}), {"a": DictSub(c=None, d=2)}))
    return cases


@needs_native
def test_rfc7386_appendix_cases():
    for target, patch, want in RFC_CASES:
        assert native.json_merge_patch(target, patch) == want
        assert kc._py_json_merge_patch(target, patch) == want


@needs_native
def test_json_merge_patch_matches_python_including_sharing():
    for target, patch in merge_inputs():
        before = (ko._py_deep_copy(target), ko._py_deep_copy(patch))
        got = native.json_merge_patch(target, patch)
        want = kc._py_json_merge_patch(target, patch)
        assert got == want
        assert (target, patch) == before  # inputs untouched
        # same sharing: a container of the result is the input's object in
        # one implementation exactly when it is in the other
        _assert_identity_pattern(got, want)


def _assert_identity_pattern(a, b):
    if a is b:
        return  # both share the same input object
    assert type(a) is type(b)
    if type(a) is dict:
        assert list(a) == list(b)
        for k in a:
            _assert_identity_pattern(a[k], b[k])
    else:
        # two distinct objects that are not fresh dicts: only possible for
        # equal scalars created independently, never for shared containers
        assert not isinstance(a, (dict, list)), "sharing differs"
        assert a == b


def reachable_mutables(tree, out=None) -> dict:
    out = {} if out is None else out
    if type(tree) in (dict, list):
        out[id(tree)] = tree
        for v in (tree.values() if type(tree) is dict else tree):
            reachable_mutables(v, out)
    return out


@pytest.mark.parametrize("impl", ["native", "python"])
def test_merge_patch_owned_equals_copy_of_merge(impl):
    if impl == "native" and native is None:
        pytest.skip("native _jsontree extension not built")
    owned = native.merge_patch_owned if impl == "native" else kc._py_merge_patch_owned
    for target, patch in merge_inputs():
        before = (ko._py_deep_copy(target), ko._py_deep_copy(patch))
        got = owned(target, patch)
        assert got == ko._py_deep_copy(kc._py_json_merge_patch(target, patch))
        assert (target, patch) == before
        # nothing mutable of the caller's patch is in the result
        mine = reachable_mutables(got)
        for oid in reachable_mutables(patch):
            assert oid not in mine


@pytest.mark.parametrize("impl", ["native", "python"])
def test_merge_patch_owned_sharing_and_ownership(impl):
    if impl == "native" and native is None:
        pytest.skip("native _jsontree extension not built")
    owned = native.merge_patch_owned if impl == "native" else kc._py_merge_patch_owned
    for patch in project_patches():
        cur = stored_nodeclaim()
        snapshot = ko._py_deep_copy(cur)
        out = owned(cur, patch)
        if not isinstance(patch, dict):
            continue
        assert out is not cur
        # every top-level subtree the patch does not name is the same object
        for k, v in cur.items():
            if k not in patch and k != "metadata":
                assert out[k] is v, k
        # inside a patched dict, untouched siblings are shared too
        if isinstance(patch.get("metadata"), dict) and "metadata" in out:
            for k, v in cur["metadata"].items():
                if k not in patch["metadata"]:
                    assert out["metadata"][k] is v, k
        if isinstance(patch.get("spec"), dict):
            assert out["spec"] is not cur["spec"]
            assert out["spec"]["requirements"] is cur["spec"]["requirements"]
            assert out["spec"]["nodeClassRef"] is cur["spec"]["nodeClassRef"]
            assert out["spec"]["resources"] is not cur["spec"]["resources"]
        # the server writes into the top level and metadata: never into cur
        out["status"] = {"clobbered": True}
        out["extra"] = 1
        if isinstance(out.get("metadata"), dict):
            assert out["metadata"] is not cur["metadata"]
            out["metadata"]["resourceVersion"] = "999"
            out["metadata"]["generation"] = 77
            out["metadata"].pop("uid", None)
        assert cur == snapshot


@needs_native
def test_merge_patch_owned_native_matches_python_sharing():
    for target, patch in merge_inputs():
        # equal results that share the same objects of `target`
        a = native.merge_patch_owned(target, patch)
        b = kc._py_merge_patch_owned(target, patch)
        assert a == b
        shared_a = set(reachable_mutables(a)) & set(reachable_mutables(target))
        shared_b = set(reachable_mutables(b)) & set(reachable_mutables(target))
        assert shared_a == shared_b


# ---------------------------------------------------------------------------
# leaks
# ---------------------------------------------------------------------------


@needs_native
def test_no_reference_or_memory_leak():
    from gpu_provisioner_amd.kube.crdschema import _compile_schema

    leaf_a, leaf_b = "leaf-a-%d" % os.getpid(), 123456789012
    tree = {"a": leaf_a, "b": [leaf_b, None, {"c": leaf_a, "d": None}], "metadata": {"x": None}}
    patch = {"b": [leaf_b, {"n": None}], "e": {"f": leaf_a, "g": None}, "a": None}
    schema = _compile_schema({
        "type": "object",
        "properties": {
            "spec": {"type": "object", "properties": {
                "a": {"type": "string", "pattern": "^leaf", "maxLength": 64},
                "q": {"anyOf": [{"type": "integer"}, {"type": "string"}], "pattern": "^[0-9]+$"},
                "l": {"type": "array", "maxItems": 4, "items": {"type": "integer", "minimum": 0}},
            }, "required": ["a"]},
        },
    })
    obj = {"spec": {"a": leaf_a, "q": "8", "l": [1, 2, leaf_b]}}
    old = {"spec": {"a": leaf_a, "q": 7, "l": [1]}}
    bad = {"spec": {"a": leaf_a, "q": "x", "l": [1]}}
    calls = [
        lambda: native.deep_copy(tree),
        lambda: native.json_merge_patch(tree, patch),
        lambda: native.merge_patch_owned(tree, patch),
        lambda: native.crd_valid(schema, obj, None, False),
        lambda: native.crd_valid(schema, obj, old, False),
        lambda: native.crd_valid(schema, bad, old, True),
    ]
    assert native.crd_valid(schema, obj, None, False) is True
    assert native.crd_valid(schema, bad, old, True) is False
    watched = (leaf_a, leaf_b, None)

    def refs():
        return [sys.getrefcount(o) for o in watched]

    for call in calls:
        call()  # first-use allocations (interned names, caches) happen here
        tracemalloc.start()
        before_refs, before_mem = refs(), tracemalloc.get_traced_memory()[0]
        for _ in range(200_000):
            call()
        after_mem = tracemalloc.get_traced_memory()[0]
        tracemalloc.stop()
        assert refs() == before_refs
        assert after_mem - before_mem < 1 << 20


# ---------------------------------------------------------------------------
# fallback
# ---------------------------------------------------------------------------

FALLBACK_SCRIPT = """
import asyncio, sys
sys.path.insert(0, %r)
from gpu_provisioner_amd.kube import objects as ko, client as kc, crdschema
from gpu_provisioner_amd.apis import v1 as karpv1
from gpu_provisioner_amd.fake.harness import Harness
print("NATIVE_JSONTREE", ko.NATIVE_JSONTREE)
assert ko.deep_copy is ko._py_deep_copy
assert kc.json_merge_patch is kc._py_json_merge_patch
assert kc.merge_patch_owned is kc._py_merge_patch_owned
assert crdschema._native_valid is None

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
    assert "NATIVE_JSONTREE False" in proc.stdout
    assert "CYCLE OK" in proc.stdout


def test_native_flag_reports_live_path():
    forced = os.environ.get("GPU_PROVISIONER_PURE_PYTHON") == "1"
    assert ko.NATIVE_JSONTREE == (native is not None and not forced)
    if ko.NATIVE_JSONTREE:
        assert ko.deep_copy is native.deep_copy
        assert kc.json_merge_patch is native.json_merge_patch
        assert kc.merge_patch_owned is native.merge_patch_owned
    else:
        assert ko.deep_copy is ko._py_deep_copy
