"""CRDValidator's native verdict walk against the pure-Python validator.

Inputs: the chart's NodeClaim CRD; the NodeClaims under examples/, what
Harness.make_nodeclaim produces, and every (new, old) pair the apiserver
validates during one provision + teardown cycle (Launched, Registered,
Initialized, status capacity, finalizer removal), plus one-field mutations
of each. The error list must be the pure-Python list exactly, native on and
native forced off, and the native verdict is "valid" exactly when that list
is empty."""
import glob
import os

import pytest
import yaml

from gpu_provisioner_amd.apis import v1 as karpv1
from gpu_provisioner_amd.fake.harness import Harness
from gpu_provisioner_amd.kube import crdschema
from gpu_provisioner_amd.kube import objects as ko
from gpu_provisioner_amd.kube.crdschema import CRDValidator
from tests.conftest import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRD_PATH = os.path.join(ROOT, "charts", "gpu-provisioner-amd", "crds", "karpenter.sh_nodeclaims.yaml")

try:
    from gpu_provisioner_amd._native import _jsontree as native
except ImportError:
    native = None

_MISSING = object()


def example_nodeclaims() -> list:
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "examples", "*.yaml"))):
        with open(path) as f:
            for doc in yaml.safe_load_all(f):
                if isinstance(doc, dict) and doc.get("kind") == karpv1.KIND_NODECLAIM:
                    out.append(doc)
    assert len(out) >= 3
    return out


def lifecycle_writes() -> list:
    """(new, old) exactly as the apiserver hands them to the validator over
    one provision + teardown cycle, identity between new and old included."""
    seen: list = []

    async def main():
        h = Harness(node_wait_interval=0.005).add_all_controllers(
            lifecycle_workers=8, termination_requeue=0.01, drain_requeue=0.01,
            instance_poll=0.01, gc_interval=30.0,
        )
        gvk = (karpv1.API_VERSION, karpv1.KIND_NODECLAIM)
        real = h.server.validators[gvk]

        def recording(new, old):
            errs = real(new, old)
            seen.append((new, old))
            return errs

        h.server.validators[gvk] = recording
        await h.start()
        try:
            await h.kube.create(h.make_nodeclaim("val1"))
            await h.wait_initialized("val1", timeout=30.0)
            await h.kube.delete(karpv1.API_VERSION, karpv1.KIND_NODECLAIM, "val1")
            await h.wait_gone(karpv1.API_VERSION, karpv1.KIND_NODECLAIM, "val1", timeout=30.0)
        finally:
            await h.stop()

    run(main())
    return seen


def with_path(tree, path: tuple, value):
    """Copy of `tree` with `path` set to `value` (or removed, for _MISSING):
    fresh containers along the path, everything else the same objects, so
    the identity a stored revision shares with its successor is kept. None
    when the path does not exist in this tree."""
    if not path:
        return value
    head, rest = path[0], path[1:]
    if isinstance(head, int):
        if not isinstance(tree, list) or len(tree) <= head:
            return None
        sub = with_path(tree[head], rest, value)
        if sub is None and rest:
            return None
        out = list(tree)
        out[head] = sub
        return out
    if not isinstance(tree, dict):
        return None
    if rest:
        if head not in tree:
            return None
        sub = with_path(tree[head], rest, value)
        if sub is None:
            return None
        return {**tree, head: sub}
    out = dict(tree)
    if value is _MISSING:
        if head not in out:
            return None
        del out[head]
    else:
        out[head] = value
    return out


MUTATIONS = [
    # wrong type
    ("type: requirements", ("spec", "requirements"), "not-a-list"),
    ("type: values", ("spec", "requirements", 0, "values"), "not-a-list"),
    ("type: nodeName", ("status", "nodeName"), 5),
    ("type: conditions", ("status", "conditions"), {"a": 1}),
    ("type: observedGeneration", ("status", "conditions", 0, "observedGeneration"), "1"),
    ("type: spec", ("spec",), []),
    # bad enum
    ("enum: operator", ("spec", "requirements", 0, "operator"), "Bogus"),
    ("enum: condition status", ("status", "conditions", 0, "status"), "Maybe"),
    # pattern miss
    ("pattern: expireAfter", ("spec", "expireAfter"), "soon"),
    ("pattern: reason", ("status", "conditions", 0, "reason"), "bad reason!"),
    ("pattern: requirement key", ("spec", "requirements", 0, "key"), "-bad/key-"),
    # over maxLength, minimum
    ("maxLength: message", ("status", "conditions", 0, "message"), "m" * 32769),
    ("maxLength: ref name", ("spec", "nodeClassRef", "name"), "n" * 254),
    ("minimum: minValues", ("spec", "requirements", 0, "minValues"), 0),
    ("maximum: minValues", ("spec", "requirements", 0, "minValues"), 51),
    ("ok: minValues", ("spec", "requirements", 0, "minValues"), 2),
    # missing required
    ("required: ref name", ("spec", "nodeClassRef", "name"), _MISSING),
    ("required: requirements", ("spec", "requirements"), _MISSING),
    ("required: condition type", ("status", "conditions", 0, "type"), _MISSING),
    # unknown field
    ("unknown: spec", ("spec", "bogusField"), 1),
    ("unknown: status", ("status", "bogusField"), {"x": 1}),
    ("unknown: condition", ("status", "conditions", 0, "bogus"), "x"),
    # bad quantity (int-or-string with a pattern on the string branch)
    ("quantity: request", ("spec", "resources", "requests", karpv1.AMD_GPU_RESOURCE), "eight"),
    ("quantity: request float", ("spec", "resources", "requests", karpv1.AMD_GPU_RESOURCE), 1.5),
    ("quantity: request int ok", ("spec", "resources", "requests", karpv1.AMD_GPU_RESOURCE), 8),
    ("quantity: capacity", ("status", "capacity", "cpu"), "lots"),
    ("quantity: allocatable", ("status", "allocatable", "memory"), ["1Gi"]),
    # changed spec on update (immutable), equal-but-not-identical spec
    ("immutable: ref name", ("spec", "nodeClassRef", "name"), "other"),
    ("immutable: requirement values", ("spec", "requirements", 0, "values"), ["Standard_Other"]),
    ("maxItems: requirements", ("spec", "requirements"),
     [{"key": "karpenter.sh/capacity-type", "operator": "In", "values": ["spot"]}] * 101),
    # CEL non-empty
    ("cel: empty ref kind", ("spec", "nodeClassRef", "kind"), ""),
]


def cases() -> list:
    """(label, new, old) for every base input and every mutation that applies."""
    h = Harness()
    base = [("example %d" % i, nc, None) for i, nc in enumerate(example_nodeclaims())]
    base.append(("make_nodeclaim", h.make_nodeclaim("made1"), None))
    writes = lifecycle_writes()
    for i, (new, old) in enumerate(writes):
        base.append(("write %d" % i, new, old))

    def conditions_true(obj) -> set:
        return {c["type"] for c in obj.get("status", {}).get("conditions", [])
                if c.get("status") == "True"}

    # the cycle did make the writes this test is about
    updates = [(n, o) for n, o in writes if o is not None]
    for cond in ("Launched", "Registered", "Initialized"):
        assert any(cond in conditions_true(n) and cond not in conditions_true(o) for n, o in updates), cond
    assert any("capacity" in n.get("status", {}) and "capacity" not in o.get("status", {}) for n, o in updates)
    assert any(ko.finalizers_of(o) and not ko.finalizers_of(n) for n, o in updates)

    out = list(base)
    for label, new, old in base:
        # an equal spec that is not the same object (deep `==` prune)
        out.append((label + " / respec", {**new, "spec": ko._py_deep_copy(new.get("spec"))}, old))
        for mlabel, path, value in MUTATIONS:
            mutated = with_path(new, path, value)
            if mutated is not None:
                out.append((f"{label} / {mlabel}", mutated, old))
    return out


@pytest.fixture(scope="module")
def all_cases():
    return cases()


def test_error_lists_and_verdict_match_python(all_cases, monkeypatch):
    validator = CRDValidator.from_file(CRD_PATH)
    n_invalid = 0
    kinds = set()
    for label, new, old in all_cases:
        # __call__ applies defaults in place on create: private top-level copies
        want = validator._violations(prepared(validator, new, old), old)
        monkeypatch.setattr(crdschema, "_native_valid", None)
        off = validator(prepared(validator, new, old, defaults=False), old)
        assert off == want, label
        if native is not None:
            monkeypatch.setattr(crdschema, "_native_valid", native.crd_valid)
            on = validator(prepared(validator, new, old, defaults=False), old)
            assert on == want, label
            verdict = native.crd_valid(
                validator.schema, prepared(validator, new, old), old, validator.spec_immutable
            )
            assert verdict is (not want), (label, want)
        n_invalid += bool(want)
        kinds.update(e.split(": ", 1)[1].split(" ")[0] for e in want)
    # the corpus is not vacuous: both outcomes, every violation kind
    assert 0 < n_invalid < len(all_cases)
    for word in ("expected", "unknown", "required", "length", "no", "spec", "may"):
        assert word in kinds, (word, sorted(kinds))


def prepared(validator: CRDValidator, new: dict, old, defaults: bool = True) -> dict:
    """A copy of `new` that a validator call may fill defaults into, sharing
    with `old` whatever `new` shares with it below the second level."""
    out = {k: (dict(v) if type(v) is dict and (old is None or v is not old.get(k)) else v)
           for k, v in new.items()}
    if defaults and old is None:
        crdschema._apply_defaults(out, validator.schema)
    return out


@pytest.mark.skipif(native is None, reason="native _jsontree extension not built")
def test_unmirrored_shapes_defer_to_python():
    """Whatever the native walk does not mirror exactly it reports as not
    valid, so the Python validator decides; __call__ stays correct."""
    validator = CRDValidator.from_file(CRD_PATH)

    class D(dict):
        pass

    h = Harness()
    nc = h.make_nodeclaim("sub1")
    nc["spec"]["nodeClassRef"] = D(nc["spec"]["nodeClassRef"])
    assert validator(nc, None) == []
    raw = {"type": "object", "properties": {"a": {"type": "string", "pattern": "^x"}}}
    assert native.crd_valid(raw, {"a": "xy"}, None, False) is False  # uncompiled pattern
    assert crdschema.validate({"a": "xy"}, raw) == []
    # an exception inside the walk is not propagated either
    bad_schema = crdschema._compile_schema(
        {"type": "object", "properties": {"n": {"type": "integer", "minimum": "1"}}}
    )
    assert native.crd_valid(bad_schema, {"n": 3}, None, False) is False
    with pytest.raises(TypeError):
        crdschema.validate({"n": 3}, bad_schema)
