"""Native revision store (native/revstore.cpp) against the Python bodies of
the in-memory apiserver's verbs it stands in for (fake/apiserver.py).

Two servers get the same calls: one whose verbs try the native entry points
first, one with the Python bodies only (`_native = None`). Returned objects,
exception types and messages, store contents, resourceVersions, history and
the events on a subscribed queue must be equal. Generated uids and timestamps
differ between two servers by nature and are masked before comparing.
Without the built extension, or with the fallback forced, the native side is
skipped by name; the Python bodies are then what the rest of the suite
already exercises."""
import asyncio
import os
import random
import re
import subprocess
import sys
import tracemalloc
from collections import OrderedDict, deque

import pytest

from gpu_provisioner_amd.fake import apiserver as fa
from gpu_provisioner_amd.fake.apiserver import InMemoryAPIServer
from gpu_provisioner_amd.fake.harness import install_chart_crd_validators
from gpu_provisioner_amd.kube import objects as ko
from gpu_provisioner_amd.kube.client import (
    AlreadyExistsError,
    ConflictError,
    InvalidError,
    NotFoundError,
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCED = os.environ.get("GPU_PROVISIONER_PURE_PYTHON") == "1"

try:
    from gpu_provisioner_amd._native import _revstore as native
except ImportError:  # not built: only the fallback tests below can run
    native = None

needs_native = pytest.mark.skipif(
    native is None or FORCED, reason="native _revstore extension not built or forced off"
)

NODE = ("v1", "Node")
CLAIM = ("karpenter.sh/v1", "NodeClaim")
EVENT = ("v1", "Event")
EVENT_CAP = 5
FIN = "karpenter.sh/termination"

_TS = re.compile(r"^\d{4}-\d\d-\d\dT\d\d:\d\d:\d\dZ$")
_UID = re.compile(r"^[0-9a-f]{8}-[0-9a-f]{4}-4[0-9a-f]{3}-[89ab][0-9a-f]{3}-[0-9a-f]{12}$")


def run(coro):
    return asyncio.run(coro)


class DictSub(dict):
    pass


def servers(validators: bool = True) -> tuple:
    """(native-first server, Python-only server), set up alike."""
    nat, ref = InMemoryAPIServer(), InMemoryAPIServer()
    nat._native, ref._native = native, None
    for s in (nat, ref):
        s._event_cap = EVENT_CAP
        if validators:
            install_chart_crd_validators(s)
    if validators:
        assert CLAIM in nat.validators, "the chart's NodeClaim CRD was not found"
    return nat, ref


def masked(tree):
    """Copy of an object with generated uids and timestamps masked."""
    if not isinstance(tree, dict) or not isinstance(tree.get("metadata"), dict):
        return tree
    out = dict(tree)
    m = out["metadata"] = dict(tree["metadata"])
    if isinstance(m.get("uid"), str) and _UID.match(m["uid"]):
        m["uid"] = "<uid>"
    for f in ("creationTimestamp", "deletionTimestamp"):
        if isinstance(m.get(f), str) and _TS.match(m[f]):
            m[f] = "<ts>"
    return out


def state(server: InMemoryAPIServer, queues: dict) -> dict:
    """Everything a write may change, masked, with queues drained."""
    events = {}
    for gvk, q in queues.items():
        got = []
        while not q.empty():
            etype, obj = q.get_nowait()
            got.append((etype, masked(obj)))
        events[gvk] = got
    return {
        "store": {g: {k: masked(v) for k, v in b.items()} for g, b in server._store.items() if b},
        "order": {g: list(b) for g, b in server._store.items() if b},
        "rv": server._rv,
        "history": [(rv, g, t, masked(o)) for rv, g, t, o in server._history],
        "events": events,
    }


async def outcome(coro):
    try:
        return ("ok", masked(await coro))
    except Exception as e:  # noqa: BLE001 - the comparison is the point
        return (type(e), str(e))


def mk_node(name: str, **meta) -> dict:
    return {
        "apiVersion": "v1", "kind": "Node",
        "metadata": {"name": name, "labels": {"agentpool": "p"}, **meta},
        "spec": {"providerID": f"azure:///{name}", "taints": [{"key": "k", "effect": "NoSchedule"}]},
        "status": {"capacity": {"cpu": "8"}, "conditions": [{"type": "Ready", "status": "False"}]},
    }


def mk_claim(name: str, **meta) -> dict:
    return {
        "apiVersion": CLAIM[0], "kind": CLAIM[1],
        "metadata": {"name": name, "labels": {"kaito.sh/workspace": "ws"}, **meta},
        "spec": {
            "requirements": [{"key": "node.kubernetes.io/instance-type", "operator": "In",
                              "values": ["Standard_ND128isr_MI355X_v6"]}],
            "resources": {"requests": {"amd.com/gpu": "8"}},
            "nodeClassRef": {"group": "kaito.sh", "kind": "KaitoNodeClass", "name": "default"},
        },
    }


def mk_event(name: str) -> dict:
    return {"apiVersion": "v1", "kind": "Event", "metadata": {"name": name, "namespace": "default"},
            "reason": "Launched", "involvedObject": {"kind": "NodeClaim", "name": name}}


# ---------------------------------------------------------------------------
# differential
# ---------------------------------------------------------------------------

NAMES = ["a", "b", "c", "d", "e"]


def random_op(rng: random.Random, step: int):
    """One operation as fn(server) -> coroutine. Everything random is drawn
    here, once, so both servers get the same call; what depends on a
    server's own revision (its uid, its current rv) is read from it."""
    gvk = rng.choice([NODE, NODE, CLAIM, CLAIM, EVENT])
    name = rng.choice(NAMES)
    ns = "default" if gvk == EVENT else ""
    kind = rng.choice(["create", "create", "update", "update", "status", "patch", "patch",
                       "status_patch", "status_patch", "delete", "get"])
    rv_mode = rng.choice(["current", "current", "none", "stale", "empty"])
    variant = rng.randrange(8)
    n = rng.randrange(1000)

    def stored(server):
        return server._store[gvk].get((ns, name))

    def with_rv(server, meta: dict) -> None:
        cur = stored(server)
        if rv_mode == "current" and cur is not None:
            meta["resourceVersion"] = cur["metadata"]["resourceVersion"]
        elif rv_mode == "stale":
            meta["resourceVersion"] = "1"
        elif rv_mode == "empty":
            meta["resourceVersion"] = ""
        else:
            meta.pop("resourceVersion", None)

    if gvk == EVENT and kind not in ("create", "get", "delete"):
        kind = "create"
    if kind == "create":
        if gvk == EVENT:
            obj = mk_event(f"ev{step}")
        else:
            extra = {}
            if variant & 1:
                extra["finalizers"] = [FIN]
            if variant & 2:
                extra["uid"] = f"u-{n}"
            if variant == 4:
                extra["creationTimestamp"] = ""
            obj = (mk_node if gvk == NODE else mk_claim)(name, **extra)
            if variant == 5:
                del obj["metadata"]["name"]
            if variant == 6 and gvk == CLAIM:
                obj["spec"]["nodeClassRef"]["name"] = ""  # CEL: may not be empty
        return lambda s: s.create(ko.deep_copy(obj))
    if kind == "get":
        return lambda s: s.get(gvk[0], gvk[1], name, ns)
    if kind == "delete":
        def call(s):
            cur = stored(s)
            uid = ""
            if variant == 0:
                uid = "not-the-uid"
            elif variant == 1 and cur is not None:
                uid = cur["metadata"]["uid"]
            return s.delete(gvk[0], gvk[1], name, ns, uid)
        return call
    if kind in ("update", "status"):
        def call(s):
            cur = stored(s)
            obj = ko.deep_copy(cur) if cur is not None else (mk_node if gvk == NODE else mk_claim)(name)
            m = obj["metadata"]
            with_rv(s, m)
            if kind == "status":
                obj["status"] = {"n": n, "conditions": [{"type": "Ready", "status": "True"}]}
                return s.update(obj, subresource="status")
            if variant == 0:
                m.setdefault("labels", {})["l"] = str(n)
            elif variant == 1:
                m["finalizers"] = list(m.get("finalizers") or []) + [f"x/{n % 3}"]
            elif variant == 2:
                m["finalizers"] = []
            elif variant == 3:
                obj["spec"] = {**obj.get("spec", {}), "providerID": f"azure:///{n}"}
            elif variant == 4:
                obj["status"] = {"ignored": True}
                m["uid"], m["generation"] = "forged", 99
                m.pop("creationTimestamp", None)
            elif variant == 5:
                obj.pop("spec", None)
            elif variant == 6:
                m["deletionTimestamp"] = "2020-01-01T00:00:00Z"
            return s.update(obj)
        return call
    # patches
    if kind == "status_patch":
        body = [
            {"status": {"n": n}},
            {"status": {"conditions": [{"type": "Ready", "status": "True", "n": n}]}},
            {"status": {"capacity": {"amd.com/gpu": "8"}, "deep": {"a": {"b": [n, {"c": n}]}}}},
            {"status": {"deep": {"a": None}, "n": None}},
            {"n": n, "bare": {"x": 1}},
            {"status": None},
            {"status": {"nodeName": f"node-{n}"}, "metadata": {}},
            {"status": {}},
        ][variant]
        sub = "status"
    else:
        body = [
            {"metadata": {"labels": {"l": str(n)}}},
            {"metadata": {"finalizers": [FIN, f"x/{n % 3}"]}},
            {"metadata": {"finalizers": None}},
            {"spec": {"providerID": f"azure:///{n}"}},
            {"metadata": {"annotations": {"a": {"nested": [n]}}}, "status": {"ignored": 1}},
            {"metadata": {"labels": None, "uid": "forged"}},
            {"spec": None},
            {},
        ][variant]
        sub = ""

    def call(s):
        patch = ko.deep_copy(body)
        if rv_mode != "none":
            with_rv(s, patch.setdefault("metadata", {}))
        return s.patch(gvk[0], gvk[1], name, patch, ns, sub)
    return call


@needs_native
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_sequences_match_python_bodies(seed):
    async def main():
        rng = random.Random(seed)
        nat, ref = servers()
        qs = [{g: s.subscribe(g[0], g[1], "")[0] for g in (NODE, CLAIM, EVENT)} for s in (nat, ref)]
        kinds = set()
        for step in range(400):
            op = random_op(rng, step)
            a, b = await outcome(op(nat)), await outcome(op(ref))
            assert a == b, f"step {step}"
            kinds.add(a[0])
            if step % 25 == 0:
                assert state(nat, qs[0]) == state(ref, qs[1]), f"step {step}"
        assert state(nat, qs[0]) == state(ref, qs[1])
        # the mix reached every outcome, and the Event cap was hit
        assert {"ok", NotFoundError, AlreadyExistsError, ConflictError, InvalidError} <= kinds
        assert len(nat._store[EVENT]) == EVENT_CAP
        assert nat._rv > 100

    run(main())


# ---------------------------------------------------------------------------
# sharing
# ---------------------------------------------------------------------------


@needs_native
def test_revisions_share_what_a_write_left_alone():
    async def main():
        nat, _ = servers(validators=False)
        await nat.create(mk_node("n", finalizers=[FIN]))
        key = ("", "n")
        rev = lambda: nat._store[NODE][key]  # noqa: E731

        old = rev()
        await nat.update({**mk_node("n"), "status": {"x": 1}}, subresource="status")
        new = rev()
        assert new is not old and new["metadata"] is not old["metadata"]
        assert new["spec"] is old["spec"]
        assert new["metadata"]["labels"] is old["metadata"]["labels"]
        assert new["metadata"]["finalizers"] is old["metadata"]["finalizers"]
        assert new["status"] == {"x": 1}

        old = new
        await nat.patch("v1", "Node", "n", {"metadata": {"labels": {"l": "1"}}}, "", "")
        new = rev()
        assert new["spec"] is old["spec"] and new["status"] is old["status"]
        assert new["metadata"]["generation"] == old["metadata"]["generation"] == 1

        old = new
        await nat.update(ko.deep_copy(old))  # equal spec: re-shared
        new = rev()
        assert new["spec"] is old["spec"]
        assert new["metadata"]["generation"] == 1

        old = new
        changed = ko.deep_copy(old)
        changed["spec"]["providerID"] = "azure:///other"
        await nat.update(changed)
        new = rev()
        assert new["spec"] is not old["spec"] and new["spec"]["providerID"] == "azure:///other"
        assert new["metadata"]["generation"] == 2

        await nat.patch("v1", "Node", "n", {"status": {"a": {"p": [1]}, "b": {"q": [2]}, "c": 3}}, "", "status")
        old = rev()
        await nat.patch("v1", "Node", "n", {"status": {"a": {"r": 1}}}, "", "status")
        new = rev()
        assert new["status"] == {"x": 1, "a": {"p": [1], "r": 1}, "b": {"q": [2]}, "c": 3}
        assert new["status"] is not old["status"] and new["status"]["a"] is not old["status"]["a"]
        assert new["status"]["b"] is old["status"]["b"]
        assert new["status"]["a"]["p"] is old["status"]["a"]["p"]
        assert new["spec"] is old["spec"]

    run(main())


# ---------------------------------------------------------------------------
# aliasing
# ---------------------------------------------------------------------------


def scribble(tree) -> None:
    """Mutate every container reachable from `tree`."""
    if type(tree) is dict:
        for v in list(tree.values()):
            scribble(v)
        tree["scribbled"] = True
    elif type(tree) is list:
        for v in tree:
            scribble(v)
        tree.append("scribbled")


@needs_native
def test_stored_revisions_alias_nothing_the_caller_holds():
    async def main():
        nat, _ = servers(validators=False)
        q, _unsub = nat.subscribe("v1", "Node", "")

        async def check(call, *inputs):
            out = await call
            snap = ko.deep_copy(nat._store[NODE][("", "n")])
            hist, (etype, queued) = ko.deep_copy(nat._history[-1][3]), q.get_nowait()
            assert queued is nat._history[-1][3] is nat._store[NODE][("", "n")]
            assert out == snap
            for tree in (*inputs, out):
                scribble(tree)
            assert nat._store[NODE][("", "n")] == snap
            assert nat._history[-1][3] == hist == snap

        obj = mk_node("n", finalizers=[FIN])
        await check(nat.create(obj), obj)
        obj = {**mk_node("n"), "status": {"deep": {"l": [1, {"m": 2}]}}}
        await check(nat.update(obj, subresource="status"), obj)
        obj = mk_node("n", labels={"x": "y"}, annotations={"a": "b"}, finalizers=[FIN])
        obj["spec"]["taints"].append({"key": "k2", "effect": "NoExecute"})
        await check(nat.update(obj), obj)
        patch = {"metadata": {"annotations": {"n": {"deep": [1, [2]]}}}, "spec": {"extra": {"l": [{}]}}}
        await check(nat.patch("v1", "Node", "n", patch, "", ""), patch)
        patch = {"status": {"deep": {"l2": [{"z": []}]}, "conditions": [{"type": "Ready", "status": "True"}]}}
        await check(nat.patch("v1", "Node", "n", patch, "", "status"), patch)
        patch = {"top": {"l": [[], {}]}}
        await check(nat.patch("v1", "Node", "n", patch, "", "status"), patch)
        got = await nat.get("v1", "Node", "n", "")
        snap = ko.deep_copy(nat._store[NODE][("", "n")])
        scribble(got)
        assert nat._store[NODE][("", "n")] == snap

    run(main())


# ---------------------------------------------------------------------------
# failures touch nothing
# ---------------------------------------------------------------------------


def fingerprint(server: InMemoryAPIServer, queues: list) -> tuple:
    return (
        {g: {k: id(v) for k, v in b.items()} for g, b in server._store.items() if b},
        ko.deep_copy({g: dict(b) for g, b in server._store.items() if b}),
        server._rv,
        [(rv, g, t, id(o)) for rv, g, t, o in server._history],
        [q.qsize() for q in queues],
    )


@needs_native
def test_failures_change_nothing_and_raise_what_python_raises():
    async def main():
        nat, ref = servers()
        queues = []
        for s in (nat, ref):
            queues.append([s.subscribe(g[0], g[1], "")[0] for g in (NODE, CLAIM)])
            await s.create(mk_node("n", uid="u-n", finalizers=[FIN]))
            await s.create(mk_claim("c", uid="u-c"))
            await s.delete("v1", "Node", "n", "")  # n is now deleting
        claim = nat._store[CLAIM][("", "c")]
        bad_spec = ko.deep_copy(claim)
        bad_spec["spec"]["resources"]["requests"]["amd.com/gpu"] = "4"  # spec is immutable
        no_name = mk_node("x")
        del no_name["metadata"]["name"]
        no_kind = mk_node("x")
        del no_kind["kind"]
        failures = {
            "get not found": (NotFoundError, lambda s: s.get("v1", "Node", "nope", "")),
            "update not found": (NotFoundError, lambda s: s.update(mk_node("nope"))),
            "patch not found": (NotFoundError, lambda s: s.patch("v1", "Node", "nope", {}, "", "")),
            "delete not found": (NotFoundError, lambda s: s.delete("v1", "Node", "nope", "")),
            "already exists": (AlreadyExistsError, lambda s: s.create(mk_node("n"))),
            "update conflict": (ConflictError, lambda s: s.update(mk_node("n", resourceVersion="1"))),
            "status conflict": (ConflictError, lambda s: s.update(
                mk_node("n", resourceVersion="1"), subresource="status")),
            "patch conflict": (ConflictError, lambda s: s.patch(
                "v1", "Node", "n", {"metadata": {"resourceVersion": "1", "labels": {"a": "b"}}}, "", "")),
            "status patch conflict": (ConflictError, lambda s: s.patch(
                "v1", "Node", "n", {"metadata": {"resourceVersion": "1"}, "status": {"a": 1}}, "", "status")),
            "finalizer 422 on update": (InvalidError, lambda s: s.update(mk_node("n", finalizers=[FIN, "new/fin"]))),
            "finalizer 422 on patch": (InvalidError, lambda s: s.patch(
                "v1", "Node", "n", {"metadata": {"finalizers": ["new/fin"]}}, "", "")),
            "validator on create": (InvalidError, lambda s: s.create(
                {**mk_claim("c2"), "spec": {"nodeClassRef": {"group": "", "kind": "K", "name": "n"}}})),
            "validator on update": (InvalidError, lambda s: s.update(ko.deep_copy(bad_spec))),
            "validator on patch": (InvalidError, lambda s: s.patch(
                CLAIM[0], CLAIM[1], "c", {"spec": {"resources": {"requests": {"amd.com/gpu": "4"}}}}, "", "")),
            "validator on status patch": (InvalidError, lambda s: s.patch(
                CLAIM[0], CLAIM[1], "c", {"status": {"conditions": "not-a-list"}}, "", "status")),
            "uid precondition": (ConflictError, lambda s: s.delete("v1", "Node", "n", "", "other-uid")),
            "missing name": (InvalidError, lambda s: s.create(ko.deep_copy(no_name))),
            "missing kind": (InvalidError, lambda s: s.create(ko.deep_copy(no_kind))),
            "missing apiVersion": (InvalidError, lambda s: s.create({"kind": "Node", "metadata": {"name": "x"}})),
        }
        for label, (exc, call) in failures.items():
            before = [fingerprint(nat, queues[0]), fingerprint(ref, queues[1])]
            a, b = await outcome(call(nat)), await outcome(call(ref))
            assert a == b and a[0] is exc, (label, a, b)
            assert fingerprint(nat, queues[0]) == before[0], label
            assert fingerprint(ref, queues[1]) == before[1], label
        # a rejected write consumed no resourceVersion on either path
        for s in (nat, ref):
            last = s._rv
            out = await s.patch(CLAIM[0], CLAIM[1], "c", {"metadata": {"labels": {"after": "x"}}}, "", "")
            assert out["metadata"]["resourceVersion"] == str(last + 1) and s._rv == last + 1
        assert nat._rv == ref._rv

    run(main())


# ---------------------------------------------------------------------------
# odd inputs go to the Python body
# ---------------------------------------------------------------------------


@needs_native
def test_odd_inputs_get_the_python_bodys_result():
    def odd_objects():
        sub = DictSub(mk_node("s"))
        ordered = OrderedDict(mk_node("o"))
        meta_sub = {**mk_node("m"), "metadata": DictSub(name="m")}
        meta_list = {**mk_node("l"), "metadata": ["name"]}
        meta_none = {**mk_node("z"), "metadata": None}
        return [sub, ordered, meta_sub, meta_list, meta_none]

    async def main():
        nat, ref = servers(validators=False)
        for i, _ in enumerate(odd_objects()):
            results = []
            for s in (nat, ref):
                obj = odd_objects()[i]
                r = [await outcome(s.create(obj))]
                r.append(await outcome(s.update(odd_objects()[i])))
                r.append(await outcome(s.update(odd_objects()[i], subresource="status")))
                results.append(r)
            assert results[0] == results[1], i
        for s in (nat, ref):
            await s.create(mk_node("p"))
        odd_patches = [DictSub(metadata={"labels": {"a": "b"}}), OrderedDict(status={"x": 1}),
                       {"metadata": DictSub(labels={"c": "d"})}, {"metadata": None}, {"metadata": "text"},
                       {"metadata": {"resourceVersion": 7}}]
        for sub in ("", "status"):
            for i, _ in enumerate(odd_patches):
                a = await outcome(nat.patch("v1", "Node", "p", ko.deep_copy(odd_patches[i]), "", sub))
                b = await outcome(ref.patch("v1", "Node", "p", ko.deep_copy(odd_patches[i]), "", sub))
                assert a == b, (sub, i)
        assert await outcome(nat.get("v1", "Node", "p", None)) == await outcome(ref.get("v1", "Node", "p", None))
        assert state(nat, {}) == state(ref, {})

    run(main())


# ---------------------------------------------------------------------------
# replaced history, resourceVersion counter
# ---------------------------------------------------------------------------


@needs_native
def test_replaced_history_and_list_resource_version():
    async def main():
        nat, ref = servers(validators=False)
        for s in (nat, ref):
            s._history = []  # a plain list in place of the deque
            await s.create(mk_node("a"))
            await s.patch("v1", "Node", "a", {"status": {"x": 1}}, "", "status")
            for _ in range(300):
                items, rv = await s.list("v1", "Node", "", "", "")
                assert rv == "2" and len(items) == 1
            out = await s.update(mk_node("a"))
            assert out["metadata"]["resourceVersion"] == "3"
            assert (await s.list("v1", "Node", "", "", ""))[1] == "3"
            assert type(s._history) is list and type(s._rv) is int
            assert [(e[0], e[2]) for e in s._history] == [(1, "ADDED"), (2, "MODIFIED"), (3, "MODIFIED")]
            assert s._history[-1][3] is s._store[NODE][("", "a")]

    run(main())


@needs_native
def test_reactors_fire_once_before_the_native_call():
    async def main():
        nat, _ = servers(validators=False)
        seen = []
        nat.reactors.append(lambda verb, gvk, payload: seen.append((verb, gvk)) or None)
        await nat.create(mk_node("a"))
        await nat.get("v1", "Node", "a", "")
        await nat.update(mk_node("a"))
        await nat.patch("v1", "Node", "a", {"status": {"x": 1}}, "", "status")
        await outcome(nat.get("v1", "Node", "nope", ""))  # falls to the Python body
        await nat.delete("v1", "Node", "a", "")
        assert seen == [(v, NODE) for v in ("create", "get", "update", "patch", "get", "delete")]

    run(main())


# ---------------------------------------------------------------------------
# leaks
# ---------------------------------------------------------------------------


@needs_native
def test_no_reference_or_memory_leak():
    native.set_helpers(ko.uuid4_str, ko.now_rfc3339)
    leaf_a, leaf_b = "leaf-a-%d" % os.getpid(), 123456789012
    server = InMemoryAPIServer()
    server._history = deque(maxlen=4)
    queue, _unsub = server.subscribe("v1", "Node", "")
    bucket = server._store[NODE]
    gvk = ("v1", "Node")

    def drain():
        while not queue.empty():
            queue.get_nowait()

    def node(name):
        return {"apiVersion": "v1", "kind": "Node",
                "metadata": {"name": name, "labels": {"l": leaf_a}, "annotations": None},
                "spec": {"v": [leaf_b, None, {"c": leaf_a}]}, "status": {"s": {"t": leaf_a}}}

    assert native.create(server, gvk, bucket, node("keep"), None, 10) is not NotImplemented
    keep, fresh, changed = node("keep"), node("fresh"), node("keep")
    changed["spec"]["v"].append(leaf_a)
    stale = node("keep")
    stale["metadata"]["resourceVersion"] = "0"
    status_patch = {"status": {"s": {"u": leaf_b, "t": None}, "w": [leaf_a, None]}}
    main_patch = {"metadata": {"labels": {"m": leaf_a, "l": None}}, "spec": {"v": [leaf_b, None]}}

    def churn():
        assert native.create(server, gvk, bucket, fresh, None, 10) is not NotImplemented
        assert native.delete(server, gvk, bucket, "", "fresh", "") is None

    def reject(new, old):
        return ["no"]

    calls = [
        churn,
        lambda: native.get(bucket, "", "keep"),
        lambda: native.update(server, gvk, bucket, keep, "", None),
        lambda: native.update(server, gvk, bucket, changed, "", None),
        lambda: native.update(server, gvk, bucket, keep, "status", None),
        lambda: native.patch(server, gvk, bucket, "", "keep", main_patch, "", None),
        lambda: native.patch(server, gvk, bucket, "", "keep", status_patch, "status", None),
        lambda: native.update(server, gvk, bucket, keep, "", lambda new, old: []),
        # sentinel paths
        lambda: native.get(bucket, "", "nope"),
        lambda: native.create(server, gvk, bucket, keep, None, 10),
        lambda: native.create(server, gvk, bucket, fresh, reject, 10),
        lambda: native.update(server, gvk, bucket, stale, "", None),
        lambda: native.update(server, gvk, bucket, keep, "", reject),
        lambda: native.update(server, gvk, bucket, DictSub(keep), "", None),
        lambda: native.patch(server, gvk, bucket, "", "nope", main_patch, "", None),
        lambda: native.patch(server, gvk, bucket, "", "keep", status_patch, "status", reject),
        lambda: native.patch(server, gvk, bucket, "", "keep", {"metadata": None}, "", None),
        lambda: native.delete(server, gvk, bucket, "", "nope", ""),
        lambda: native.delete(server, gvk, bucket, "", "keep", "other-uid"),
    ]
    for call in calls[8:]:
        assert call() is NotImplemented
    watched = (leaf_a, leaf_b, None, NotImplemented, gvk)

    def refs():
        return [sys.getrefcount(o) for o in watched]

    for i, call in enumerate(calls):
        for _ in range(4):  # first-use allocations, and the history ring turns over
            call()
        drain()
        tracemalloc.start()
        before_refs, before_mem = refs(), tracemalloc.get_traced_memory()[0]
        for _ in range(20_000):
            call()
            drain()
        after_mem = tracemalloc.get_traced_memory()[0]
        tracemalloc.stop()
        assert refs() == before_refs, i
        assert after_mem - before_mem < 1 << 20, i


# ---------------------------------------------------------------------------
# fallback
# ---------------------------------------------------------------------------

FALLBACK_SCRIPT = """
import asyncio, sys
sys.path.insert(0, %r)
from gpu_provisioner_amd.fake import apiserver as fa
from gpu_provisioner_amd.apis import v1 as karpv1
from gpu_provisioner_amd.fake.harness import Harness
print("NATIVE_REVSTORE", fa.NATIVE_REVSTORE)
assert fa._native_revstore is None

async def cycle():
    h = Harness(node_wait_interval=0.005).add_all_controllers(
        lifecycle_workers=8, termination_requeue=0.01, drain_requeue=0.01,
        instance_poll=0.01, gc_interval=30.0)
    assert h.server._native is None
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
    assert "NATIVE_REVSTORE False" in proc.stdout
    assert "CYCLE OK" in proc.stdout


def test_native_flag_reports_live_path():
    assert fa.NATIVE_REVSTORE == (native is not None and not FORCED)
    assert InMemoryAPIServer()._native is (native if fa.NATIVE_REVSTORE else None)


def test_python_bodies_keep_the_counter_an_integer():
    """The fallback alone: many list() calls leave the counter a plain int
    that reads back the last issued resourceVersion."""
    async def main():
        s = InMemoryAPIServer()
        s._native = None
        await s.create(mk_node("a"))
        for _ in range(300):
            assert (await s.list("v1", "Node", "", "", ""))[1] == "1"
        out = await s.update(mk_node("a"), subresource="status")
        assert out["metadata"]["resourceVersion"] == "2" and s._rv == 2
        assert [e[0] for e in s._history] == [1, 2]

    run(main())
