#!/usr/bin/env python3
"""Benchmark: NodeClaim provisioning throughput + p50 Ready latency.

Measures BASELINE.json's north-star metric on config #1 ("Single NodeClaim
reconciled against fake cloudprovider — CPU-only plumbing, no cloud"): the
full controller stack (in-memory apiserver + informers + lifecycle controller
+ instance provider + fake AKS with zero cloud latency) provisioning and
tearing down batches of MI355X NodeClaims. One *step* = provision
`--concurrent` NodeClaims to Initialized (amd.com/gpu registered), then
delete them to completion (full churn cycle). The reference (Azure/
gpu-provisioner) publishes no numbers, so vs_baseline is null;
the implicit envelope to beat is its fixed per-claim overhead (≥1 s
post-patch sleep on the provision path + 5 s termination polls).

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--concurrent C]
                       [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints one JSON result
line; nothing else is measured. On a host with a GPU, setup asks the native
node agent which device that is (discovery only, no kernel launch) and names
it in the result's config block. --dump-outputs DIR additionally writes what
the last timed step produced (see dump_outputs) as DIR/<name>.npy so two
builds can be compared output for output. --full is reserved for
measurements beyond the headline figure (there are none today).
For N>1 the driver launches this under torch.distributed.run, one rank per
GPU; the workload is controller plumbing (CPU-bound), ranks run independent
provisioner stacks and aggregate via gloo (weak scaling).
"""
from __future__ import annotations

import argparse
import asyncio
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_provisioner_amd.apis import v1 as karpv1  # noqa: E402
from gpu_provisioner_amd.fake.harness import Harness  # noqa: E402

VM_SIZE = "Standard_ND128isr_MI355X_v6"


def build_harness(create_latency: float = 0.0, ready_latency: float = 0.0) -> Harness:
    # the full production controller topology: lifecycle + termination +
    # eviction + both GCs (health excluded: no repairs during a clean bench)
    # progress is event-driven (node/pod/VA events re-trigger reconciles);
    # the requeue intervals are BACKSTOPS. Sub-10ms backstops busy-poll and
    # livelock the loop at high concurrency (128+ claims).
    return Harness(
        create_latency=create_latency,
        ready_latency=ready_latency,
        # node-wait polls hit the informer cache (zero-copy dict lookups),
        # so a tight interval is cheap; 10ms quantized p50 Ready visibly
        node_wait_interval=0.002,
    ).add_all_controllers(
        lifecycle_workers=256,
        termination_workers=128,
        termination_requeue=0.02,
        drain_requeue=0.02,
        instance_poll=0.02,
        gc_interval=30.0,
        with_health=False,
    )


async def one_step(h: Harness, step: int, concurrent: int, latencies: list) -> dict:
    """One churn cycle. Returns what a caller of the cycle receives: the
    Initialized NodeClaims (in name order) and, per claim, whether its
    deletion was observed to completion."""
    names = [f"s{step % 1000:03d}c{i:02d}" for i in range(concurrent)]

    async def provision(name: str) -> dict:
        t0 = time.monotonic()
        await h.kube.create(h.make_nodeclaim(name, VM_SIZE))
        nc = await h.wait_initialized(name, timeout=60.0, interval=0.001)
        latencies.append(time.monotonic() - t0)
        return nc

    claims = await asyncio.gather(*(provision(n) for n in names))

    async def teardown(name: str) -> bool:
        await h.kube.delete(karpv1.API_VERSION, karpv1.KIND_NODECLAIM, name)
        return bool(
            await h.wait_gone(karpv1.API_VERSION, karpv1.KIND_NODECLAIM, name, timeout=60.0, interval=0.001)
        )

    gone = await asyncio.gather(*(teardown(n) for n in names))
    return {"claims": list(claims), "gone": list(gone)}


RESOURCE_NAMES = ("cpu", "memory", "ephemeral-storage", "pods", karpv1.AMD_GPU_RESOURCE)
CONDITION_TYPES = ("Launched", "Registered", "Initialized", "Ready")
_QUANTITY_SUFFIXES = {
    "Ki": 2.0**10, "Mi": 2.0**20, "Gi": 2.0**30, "Ti": 2.0**40, "Pi": 2.0**50, "Ei": 2.0**60,
    "m": 1e-3, "k": 1e3, "M": 1e6, "G": 1e9, "T": 1e12, "P": 1e15, "E": 1e18,
}


def quantity_to_float(q) -> float:
    """Kubernetes resource quantity ("128", "2036Gi", "500m") as a float;
    NaN when absent."""
    if q is None:
        return float("nan")
    q = str(q)
    for suffix in sorted(_QUANTITY_SUFFIXES, key=len, reverse=True):
        if q.endswith(suffix):
            return float(q[: -len(suffix)]) * _QUANTITY_SUFFIXES[suffix]
    return float(q)


MAX_DUMP_BYTES = 64 * 1000 * 1000
# float64 columns per claim: 5 + 5 resources, 4 conditions, 5 identity, 2 labels, 1 gone
DUMP_BYTES_PER_CLAIM = 8 * (2 * len(RESOURCE_NAMES) + len(CONDITION_TYPES) + 5 + 2 + 1)


def dump_outputs(out_dir: str, last: dict) -> None:
    """Write the last timed step's results as float64 .npy arrays, one row
    per NodeClaim in name order. Only run-invariant fields are kept (no
    UIDs, timestamps or resourceVersions), so equal arguments give equal
    files (MAX_DUMP_BYTES in all; a step with more claims than fit is cut
    to a fixed, seeded sample of its rows, kept in name order):

      capacity.npy / allocatable.npy  [claims, 5]  status quantities, columns
                                      RESOURCE_NAMES (bytes for memory/storage)
      conditions.npy                  [claims, 4]  CONDITION_TYPES; 1 True,
                                      0 otherwise, -1 condition absent
      identity.npy                    [claims, 5]  CRC-32 of name, nodeName,
                                      providerID, instance-type and
                                      capacity-type labels
      labels.npy                      [claims, 2]  amd.com/gpu.count label,
                                      number of labels carrying the amd.com/ prefix
      gone.npy                        [claims]     1 if deletion completed
    """
    import zlib

    import numpy as np

    claims, gone = last["claims"], last["gone"]
    # six files, each with a 128-byte .npy header
    keep = (MAX_DUMP_BYTES - 6 * 128) // DUMP_BYTES_PER_CLAIM
    if len(claims) > keep:
        rows = sorted(np.random.default_rng(0).choice(len(claims), size=keep, replace=False))
        claims, gone = [claims[i] for i in rows], [gone[i] for i in rows]

    def crc(text) -> float:
        return float(zlib.crc32(str(text or "").encode()))

    def resources(nc: dict, field: str):
        quantities = nc.get("status", {}).get(field, {})
        return [quantity_to_float(quantities.get(r)) for r in RESOURCE_NAMES]

    def conditions(nc: dict):
        by_type = {c.get("type"): c.get("status") for c in nc.get("status", {}).get("conditions", [])}
        return [
            -1.0 if t not in by_type else (1.0 if by_type[t] == "True" else 0.0)
            for t in CONDITION_TYPES
        ]

    def identity(nc: dict):
        labels = nc["metadata"].get("labels", {})
        status = nc.get("status", {})
        return [
            crc(nc["metadata"]["name"]),
            crc(status.get("nodeName")),
            crc(status.get("providerID")),
            crc(labels.get(karpv1.INSTANCE_TYPE_LABEL_KEY)),
            crc(labels.get("karpenter.sh/capacity-type")),
        ]

    def label_facts(nc: dict):
        labels = nc["metadata"].get("labels", {})
        return [
            quantity_to_float(labels.get("amd.com/gpu.count")),
            float(sum(1 for k in labels if k.startswith("amd.com/"))),
        ]

    arrays = {
        "capacity": [resources(nc, "capacity") for nc in claims],
        "allocatable": [resources(nc, "allocatable") for nc in claims],
        "conditions": [conditions(nc) for nc in claims],
        "identity": [identity(nc) for nc in claims],
        "labels": [label_facts(nc) for nc in claims],
        "gone": [1.0 if g else 0.0 for g in gone],
    }
    os.makedirs(out_dir, exist_ok=True)
    for name, rows in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), np.asarray(rows, dtype=np.float64))


async def run_bench(
    steps: int, warmup: int, concurrent: int,
    create_latency: float = 0.0, ready_latency: float = 0.0,
    rss_every: int = 0,
) -> dict:
    h = build_harness(create_latency, ready_latency)
    await h.start()
    try:
        rss: list = []

        def sample_rss(step: int) -> None:
            # soak-memory evidence: flat RSS over long
            # runs is the leak check the reference covers with its heap
            # profile endpoint
            if rss_every and step % rss_every == 0:
                import psutil

                rss.append(
                    {"step": step, "rss_bytes": psutil.Process().memory_info().rss}
                )

        warm_lat: list = []
        for s in range(warmup):
            await one_step(h, s, concurrent, warm_lat)
        latencies: list = []
        last: dict = {"claims": [], "gone": []}
        t0 = time.monotonic()
        for s in range(warmup, warmup + steps):
            sample_rss(s)
            last = await one_step(h, s, concurrent, latencies)
        sample_rss(warmup + steps)
        elapsed = time.monotonic() - t0
        return {"elapsed_s": elapsed, "latencies": latencies, "rss": rss, "last": last}
    finally:
        await h.stop()


def identify_device(gpu_present: bool, rank: int = 0):
    """Which device a figure was measured next to, as the native node agent
    (the gfx950 HIP library) discovers it: index, name, arch, HBM size and
    CU count. Discovery only, no kernel is launched. A host without a GPU
    has no device and the library is not touched. The figure does not depend
    on the answer, so a missing library or a failed query does not stop the
    run: it is reported on stderr and recorded as {"error": ...}."""
    if not gpu_present:
        return None
    from gpu_provisioner_amd.nodeagent import NodeAgent, NodeAgentError

    try:
        agent = NodeAgent()
        dev = rank % agent.device_count()
        name, arch, hbm, cus = agent.device_info(dev)
    except NodeAgentError as e:
        print(f"bench: device not identified: {e}", file=sys.stderr)
        return {"error": str(e)}
    return {"index": dev, "name": name, "arch": arch, "hbm_gb": round(hbm / 1e9, 1), "cus": cus}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--concurrent", type=int, default=8,
                    help="NodeClaims provisioned per step (8 = one full MI355X host worth)")
    ap.add_argument("--create-latency", type=float, default=0.0,
                    help="simulated agent-pool LRO seconds (0 = BASELINE config #1)")
    ap.add_argument("--ready-latency", type=float, default=0.0,
                    help="simulated node boot-to-Ready seconds")
    ap.add_argument("--rss-out", default="",
                    help="write per-step RSS samples (soak memory evidence) to this JSON file")
    ap.add_argument("--rss-every", type=int, default=100,
                    help="sample RSS every N steps when --rss-out is set")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write the last step's results as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run measurements beyond the headline figure "
                         "(none exist today; a plain run is already minimal)")
    args = ap.parse_args()

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dist = None
    if world_size > 1:
        import torch.distributed as dist  # type: ignore

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo", rank=rank, world_size=world_size)

    try:
        import torch

        cuda = torch.cuda.is_available()
    except Exception:
        torch, cuda = None, False

    def sync():
        if dist is not None:
            dist.barrier()
        if cuda:
            torch.cuda.synchronize()

    sync()
    device = identify_device(cuda, rank)
    result = asyncio.run(
        run_bench(
            args.steps, args.warmup, args.concurrent,
            args.create_latency, args.ready_latency,
            rss_every=(args.rss_every if args.rss_out else 0),
        )
    )
    sync()
    if args.rss_out and rank == 0:
        rss = result.get("rss", [])
        summary = {
            "steps": args.steps,
            "concurrent": args.concurrent,
            "samples": rss,
            "rss_first_bytes": rss[0]["rss_bytes"] if rss else None,
            "rss_last_bytes": rss[-1]["rss_bytes"] if rss else None,
            "rss_max_bytes": max((s["rss_bytes"] for s in rss), default=None),
        }
        with open(args.rss_out, "w") as f:
            json.dump(summary, f, indent=1)

    if args.dump_outputs and rank == 0:
        # rank 0's own stack; every rank runs the same deterministic workload
        dump_outputs(args.dump_outputs, result["last"])

    elapsed = result["elapsed_s"]
    if dist is not None:
        import torch as _t

        buf = _t.tensor([elapsed], dtype=_t.float64)
        dist.all_reduce(buf, op=dist.ReduceOp.MAX)
        max_elapsed = float(buf.item())
        all_lat: list = [None] * world_size
        dist.all_gather_object(all_lat, result["latencies"])
        latencies = [x for part in all_lat for x in part]
    else:
        max_elapsed = elapsed
        latencies = result["latencies"]

    total_claims = args.steps * args.concurrent * world_size
    value = total_claims / (max_elapsed / 60.0)
    p50 = statistics.median(latencies) if latencies else float("nan")
    p95 = (
        statistics.quantiles(latencies, n=20)[18]
        if len(latencies) >= 20
        else (max(latencies) if latencies else float("nan"))
    )
    p99 = (
        statistics.quantiles(latencies, n=100)[98]
        if len(latencies) >= 100
        else (max(latencies) if latencies else float("nan"))
    )

    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": "nodeclaims_per_min",
                    "value": round(value, 2),
                    "unit": "NodeClaims/min",
                    "n_gpus": world_size,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": round(max_elapsed / args.steps * 1000.0, 3),
                    "higher_is_better": True,
                    "scaling": "weak",
                    "vs_baseline": None,
                    "dtype": "n/a",
                    "data": "synthetic",
                    "config": {
                        "model": "MI355X NodeClaim provisioning (karpenter CloudProvider contract)",
                        "vm_sku": VM_SIZE,
                        "concurrent_nodeclaims": args.concurrent,
                        # rank 0's device as seen by the native node agent
                        "device": device,
                        "cloud": (
                            "in-memory fake AKS, zero latency (BASELINE config #1)"
                            if not (args.create_latency or args.ready_latency)
                            else (
                                f"in-memory fake AKS, simulated LRO {args.create_latency}s"
                                f" + node-ready {args.ready_latency}s"
                            )
                        ),
                        # round-2 apiserver realism: every write is admission-
                        # validated against the chart's CRD schemas in-process
                        # (r01 benches had no admission — numbers compare
                        # accordingly)
                        "apiserver": "in-memory, server-side CRD validation on",
                        "cycle": "create→Launched→Registered→Initialized(amd.com/gpu)→delete→gone",
                        "p50_ready_latency_s": round(p50, 4),
                        "p95_ready_latency_s": round(p95, 4),
                        "p99_ready_latency_s": round(p99, 4),
                        "parallelism": f"dp{world_size}" if world_size > 1 else "single",
                    },
                }
            )
        )
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
