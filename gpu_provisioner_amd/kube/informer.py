"""Informer: list+watch cache with indexers and event handlers.

Replaces the controller-runtime cache + field indexers the reference registers
in vendor/sigs.k8s.io/karpenter/pkg/operator/operator.go:250-293 (pod by
spec.nodeName, node by spec.providerID, nodeclaim by status.providerID,
volumeattachment by spec.nodeName). Handlers are invoked for every event and
typically enqueue keys onto a controller's workqueue.
"""
from __future__ import annotations

import asyncio
import logging
from collections import defaultdict
from typing import Callable, Optional

from . import objects as ko
from .client import ADDED, BOOKMARK, DELETED, GoneError, KubeClient, MODIFIED

log = logging.getLogger(__name__)


def _py_object_key(obj: dict) -> str:
    ns = ko._py_namespace_of(obj)
    return f"{ns}/{ko._py_name_of(obj)}" if ns else ko._py_name_of(obj)


def _py_field_index(*paths) -> Callable:
    """Index function over fixed key paths, e.g. ("spec", "providerID") or
    the two ("metadata", "labels", <key>) paths of the agentpool index.
    Follows add_index's contract: None for no value, otherwise the list of
    non-empty values found at the paths, in path order. The top-level
    section is read as obj.get(k, {}), deeper maps as .get(k) or {}. On an
    object that breaks the wire format it does what the lambdas it replaced
    did: a missing-but-not-absent section raises, and a single path whose
    value is not a string gives that value itself for add_index to iterate."""
    paths = tuple(tuple(p) for p in paths)

    def index(obj: dict):
        out = []
        for path in paths:
            cur = obj
            for depth, k in enumerate(path[:-1]):
                cur = cur.get(k, {}) if depth == 0 else (cur.get(k) or {})
            v = cur.get(path[-1])
            if v:
                if len(paths) == 1 and not isinstance(v, str):
                    return v
                out.append(v)
        return out or None

    return index


def _py_index_store(key: str, old: Optional[dict], new: Optional[dict], indexes: dict, cache: dict) -> None:
    """Replace revision `old` of `key` by `new` in the index buckets and the
    cache; either may be None (ADDED: no old, DELETED: no new)."""
    for obj, remove in ((old, True), (new, False)):
        if obj is None:
            if not remove:
                cache.pop(key, None)
            continue
        if not remove:
            cache[key] = obj
        for fn, idx in indexes.values():
            vals = fn(obj)
            if vals is None:
                continue
            if isinstance(vals, str):
                vals = [vals]
            for v in vals:
                if remove:
                    s = idx.get(v)
                    if s is not None:
                        s.discard(key)
                        # drop emptied buckets: a defaultdict(set) keeps one
                        # empty set per index value EVER seen, which is an
                        # unbounded live-object leak at churn (measured
                        # ~5 sets/claim, +260 MB RSS over a 20k-step soak)
                        if not s:
                            del idx[v]
                else:
                    idx[v].add(key)


# native/objmodel.cpp replaces the three helpers above when it has been built
# (ko.NATIVE_OBJMODEL). Its index_store runs every index function on both
# revisions first and touches the buckets only where the values differ:
# providerID, nodeName and the agentpool labels are write-once, so nearly
# every MODIFIED event leaves the indexes alone.
if ko.NATIVE_OBJMODEL:
    ko._native_objmodel.set_fallbacks({"object_key": _py_object_key})
    object_key = ko._native_objmodel.object_key
    _index_store = ko._native_objmodel.index_store

    def field_index(*paths) -> Callable:
        return ko._native_objmodel.field_index(_py_field_index(*paths), *paths)

else:
    object_key = _py_object_key
    _index_store = _py_index_store
    field_index = _py_field_index
field_index.__doc__ = _py_field_index.__doc__


class Informer:
    """Cache for one (apiVersion, kind), kept fresh by a list+watch loop."""

    def __init__(
        self,
        client: KubeClient,
        api_version: str,
        kind: str,
        namespace: str = "",
        label_selector: str = "",
        resync_period: float = 0.0,
    ):
        self.client = client
        self.api_version = api_version
        self.kind = kind
        self.namespace = namespace
        self.label_selector = label_selector
        self.resync_period = resync_period
        self._cache: dict = {}  # key -> obj
        self._indexes: dict = {}  # index_name -> (fn, {value: set(keys)})
        self._handlers: list = []  # fn(event_type, obj)
        self._key_waiters: dict = {}  # key -> [(predicate, future)]
        self._index_waiters: dict = {}  # index -> {value: [(predicate, future)]}
        self._synced = asyncio.Event()
        self._task: Optional[asyncio.Task] = None
        self._rv = ""

    # -- registration -------------------------------------------------------

    def add_index(self, name: str, fn: Callable) -> None:
        """fn(obj) -> Optional[str] | list[str]: index value(s) for the object.
        Idempotent: re-registering an existing index name is a no-op.

        Like add_handler's replay, an index registered after sync is
        backfilled from the current cache — a late-bound index (e.g. via
        set_nodes_informer) must not silently return empty by_index results."""
        if name in self._indexes:
            return
        idx: defaultdict = defaultdict(set)
        self._indexes[name] = (fn, idx)
        for key, obj in self._cache.items():
            vals = fn(obj)
            if vals is None:
                continue
            if isinstance(vals, str):
                vals = [vals]
            for v in vals:
                idx[v].add(key)

    def has_index(self, name: str) -> bool:
        return name in self._indexes

    def add_handler(self, fn: Callable) -> None:
        """fn(event_type, obj) — called for ADDED/MODIFIED/DELETED.

        client-go semantics: the current store is replayed to the new
        handler as synthetic ADDED events, so a handler registered after
        sync (e.g. a restarted controller) still sees the whole world —
        level-triggered recovery depends on this."""
        self._handlers.append(fn)
        for obj in list(self._cache.values()):
            try:
                fn(ADDED, obj)
            except Exception:
                log.exception("informer %s handler failed during replay", self.kind)

    def remove_handler(self, fn: Callable) -> None:
        try:
            self._handlers.remove(fn)
        except ValueError:
            pass

    # -- keyed waiters --------------------------------------------------------
    #
    # A parked plain handler costs O(waiters) per event; at a few hundred
    # concurrent waiters that dominated the profile. Keyed waiters dispatch
    # in O(1): by object key, or by an index value (e.g. the agentpool
    # label) when the object's name isn't known in advance.

    async def wait_until(
        self,
        predicate: Callable,
        *,
        name: str = "",
        namespace: str = "",
        index: str = "",
        value: str = "",
        timeout: float = 10.0,
    ):
        """Await predicate(event_type, obj) returning non-None for events on
        ONE key — an object name or an (index, value) pair. The current
        cache state is checked first (event_type "ADDED", or "ABSENT" with
        obj=None for a missing name)."""
        if name:
            key = f"{namespace}/{name}" if namespace else name
            obj = self._cache.get(key)
            res = predicate("ADDED" if obj is not None else "ABSENT", obj)
            if res is not None:
                return res
            waiters = self._key_waiters.setdefault(key, [])
        else:
            _, idx = self._indexes[index]
            for k in list(idx.get(value, ())):
                obj = self._cache.get(k)
                if obj is not None:
                    res = predicate("ADDED", obj)
                    if res is not None:
                        return res
            waiters = self._index_waiters.setdefault(index, {}).setdefault(value, [])

        fut: asyncio.Future = asyncio.get_running_loop().create_future()
        entry = (predicate, fut)
        waiters.append(entry)
        try:
            return await asyncio.wait_for(fut, timeout)
        finally:
            try:
                waiters.remove(entry)
            except ValueError:
                pass
            # drop empty registries: one leftover list per key/value ever
            # waited on is a slow leak at churn rates
            if not waiters:
                if name:
                    self._key_waiters.pop(key, None)
                else:
                    vmap = self._index_waiters.get(index)
                    if vmap is not None:
                        vmap.pop(value, None)
                        if not vmap:
                            self._index_waiters.pop(index, None)

    def _fire_waiters(self, waiters: Optional[list], event_type: str, obj: dict) -> None:
        if not waiters:
            return
        for pred, fut in list(waiters):
            if fut.done():
                continue
            try:
                res = pred(event_type, obj)
            except Exception:
                log.exception("informer %s waiter predicate failed", self.kind)
                continue
            if res is not None:
                fut.set_result(res)

    def _dispatch_waiters(self, event_type: str, obj: dict) -> None:
        if self._key_waiters:
            self._fire_waiters(self._key_waiters.get(object_key(obj)), event_type, obj)
        if self._index_waiters:
            for index, wmap in self._index_waiters.items():
                fn, _ = self._indexes[index]
                vals = fn(obj)
                if vals is None:
                    continue
                if isinstance(vals, str):
                    vals = [vals]
                for v in vals:
                    self._fire_waiters(wmap.get(v), event_type, obj)

    # -- cache access -------------------------------------------------------
    #
    # Shared-object contract (client-go parity): objects returned from the
    # cache are SHARED and read-only. A caller that wants to mutate must
    # ko.deep_copy() first — in practice controllers re-read via the kube
    # client (which returns private copies) before any write. Copying here
    # was 40% of the provisioning-path profile.

    def get(self, name: str, namespace: str = "") -> Optional[dict]:
        key = f"{namespace}/{name}" if namespace else name
        return self._cache.get(key)

    def list(self) -> list:
        return list(self._cache.values())

    def by_index(self, index: str, value: str) -> list:
        _, idx = self._indexes[index]
        return [self._cache[k] for k in idx.get(value, set()) if k in self._cache]

    async def wait_for_sync(self) -> None:
        await self._synced.wait()

    @property
    def has_synced(self) -> bool:
        return self._synced.is_set()

    # -- run loop -----------------------------------------------------------

    def start(self) -> asyncio.Task:
        if self._task is None:
            self._task = asyncio.create_task(self._run(), name=f"informer-{self.kind}")
            if self.resync_period > 0:
                self._resync_task = asyncio.create_task(
                    self._resync_loop(), name=f"informer-resync-{self.kind}"
                )
        return self._task

    async def stop(self) -> None:
        for attr in ("_task", "_resync_task"):
            task = getattr(self, attr, None)
            if task:
                task.cancel()
                try:
                    await task
                except (asyncio.CancelledError, Exception):
                    pass
                setattr(self, attr, None)

    async def _resync_loop(self) -> None:
        """client-go resync: periodically re-deliver every cached object as
        MODIFIED so level-triggered controllers recover from any missed or
        mishandled event."""
        while True:
            await asyncio.sleep(self.resync_period)
            for obj in list(self._cache.values()):
                self._notify(MODIFIED, obj)

    async def _run(self) -> None:
        backoff = 0.05
        while True:
            try:
                await self._list_and_watch()
                backoff = 0.05
            except asyncio.CancelledError:
                raise
            except GoneError:
                self._rv = ""  # force full relist
                continue
            except Exception:
                log.exception("informer %s list/watch failed; retrying in %.2fs", self.kind, backoff)
                await asyncio.sleep(backoff)
                backoff = min(backoff * 2, 5.0)

    async def _list_and_watch(self) -> None:
        # list
        if hasattr(self.client, "list_with_rv"):
            items, rv = await self.client.list_with_rv(  # type: ignore[attr-defined]
                self.api_version, self.kind, self.namespace, self.label_selector
            )
        else:
            items = await self.client.list(
                self.api_version, self.kind, self.namespace, self.label_selector
            )
            rv = max((int(o["metadata"].get("resourceVersion", 0)) for o in items), default=0)
            rv = str(rv)
        self._rv = rv
        new_keys = {object_key(o) for o in items}
        # deletions that happened while we weren't watching
        for key in list(self._cache):
            if key not in new_keys:
                gone = self._cache[key]
                _index_store(key, gone, None, self._indexes, self._cache)
                self._notify(DELETED, gone)
        for obj in items:
            self._store(obj, event=MODIFIED if object_key(obj) in self._cache else ADDED)
        self._synced.set()
        # watch
        async for event_type, obj in self.client.watch(
            self.api_version, self.kind, self.namespace, self._rv, self.label_selector
        ):
            self._rv = obj.get("metadata", {}).get("resourceVersion", self._rv)
            if event_type == BOOKMARK:
                continue  # rv advanced above; no object state change
            if event_type == DELETED:
                key = object_key(obj)
                old = self._cache.get(key)
                _index_store(key, old or obj, None, self._indexes, self._cache)
                self._notify(DELETED, obj)
            else:
                self._store(obj, event=event_type)

    def _store(self, obj: dict, event: str) -> None:
        key = object_key(obj)
        _index_store(key, self._cache.get(key), obj, self._indexes, self._cache)
        self._notify(event, obj)

    def _notify(self, event_type: str, obj: dict) -> None:
        for h in self._handlers:
            try:
                h(event_type, obj)
            except Exception:
                log.exception("informer %s handler failed", self.kind)
        self._dispatch_waiters(event_type, obj)


class InformerFactory:
    """One shared informer per (apiVersion, kind, selector)."""

    def __init__(self, client: KubeClient):
        self.client = client
        self._informers: dict = {}

    def informer(
        self, api_version: str, kind: str, namespace: str = "", label_selector: str = ""
    ) -> Informer:
        key = (api_version, kind, namespace, label_selector)
        if key not in self._informers:
            self._informers[key] = Informer(self.client, api_version, kind, namespace, label_selector)
        return self._informers[key]

    def start_all(self) -> list:
        return [inf.start() for inf in self._informers.values()]

    async def wait_for_sync(self) -> None:
        await asyncio.gather(*(inf.wait_for_sync() for inf in self._informers.values()))

    async def stop_all(self) -> None:
        for inf in self._informers.values():
            await inf.stop()
