"""bench.py --dump-outputs: the last timed step's results land as float
.npy arrays that are identical from run to run, so two builds can be
compared output for output."""
import asyncio
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAMES = ("capacity", "allocatable", "conditions", "identity", "labels", "gone")


def _dump(out_dir, steps=2, warmup=1, concurrent=3):
    result = asyncio.run(bench.run_bench(steps, warmup, concurrent))
    bench.dump_outputs(str(out_dir), result["last"])
    return {n: np.load(os.path.join(str(out_dir), f"{n}.npy")) for n in NAMES}


def test_dump_outputs_content_and_determinism(tmp_path):
    a = _dump(tmp_path / "a")
    b = _dump(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in NAMES)
    for n in NAMES:
        assert a[n].dtype == np.float64
        assert a[n].shape[0] == 3
        assert np.array_equal(a[n], b[n]), n
    # one MI355X host per claim: 8 GPUs, 128 vCPU, 2048 GiB; all four
    # conditions True; deletion observed to completion
    cols = {r: i for i, r in enumerate(bench.RESOURCE_NAMES)}
    assert (a["capacity"][:, cols["amd.com/gpu"]] == 8).all()
    assert (a["capacity"][:, cols["cpu"]] == 128).all()
    assert (a["capacity"][:, cols["memory"]] == 2048 * 2.0**30).all()
    assert (a["allocatable"] <= a["capacity"]).all()
    assert (a["conditions"] == 1.0).all()
    assert (a["labels"][:, 0] == 8).all()
    assert (a["gone"] == 1.0).all()
    # distinct claims have distinct names, nodes and provider IDs
    for col in range(3):
        assert len(set(a["identity"][:, col])) == 3


def test_dump_outputs_respects_size_ceiling(tmp_path, monkeypatch):
    """More claims than fit under the ceiling are cut to the same seeded
    sample of rows every time, in name order."""
    last = asyncio.run(bench.run_bench(1, 0, 6))["last"]
    monkeypatch.setattr(bench, "MAX_DUMP_BYTES", 4 * bench.DUMP_BYTES_PER_CLAIM + 6 * 128)
    full_names = [float(zlib.crc32(nc["metadata"]["name"].encode()))
                  for nc in last["claims"]]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), last)
    a, b = (
        {n: np.load(os.path.join(str(tmp_path / d), f"{n}.npy")) for n in NAMES} for d in ("a", "b")
    )
    on_disk = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f"{n}.npy")) for n in NAMES)
    assert on_disk <= bench.MAX_DUMP_BYTES
    for n in NAMES:
        assert a[n].shape[0] == 4
        assert np.array_equal(a[n], b[n])
    kept = [full_names.index(v) for v in a["identity"][:, 0]]
    assert kept == sorted(kept) and len(set(kept)) == 4


def test_no_gpu_means_no_device_and_no_native_library(monkeypatch):
    """A host without a GPU runs the benchmark without the HIP build."""
    import gpu_provisioner_amd.nodeagent as na

    def boom():
        raise AssertionError("library must not be loaded without a GPU")

    monkeypatch.setattr(na, "_load_lib", boom)
    assert bench.identify_device(False) is None


def test_unidentified_device_is_recorded_not_fatal(monkeypatch, capsys):
    """A missing node-agent library on a GPU host must not stop the run."""
    import gpu_provisioner_amd.nodeagent as na

    def missing():
        raise na.NodeAgentError("libmi355x_nodeagent.so not found")

    monkeypatch.setattr(na, "_load_lib", missing)
    assert bench.identify_device(True) == {"error": "libmi355x_nodeagent.so not found"}
    assert "device not identified" in capsys.readouterr().err


@pytest.mark.gpu
def test_identify_device_reports_mi355x():
    device = bench.identify_device(True)
    assert device["index"] == 0
    assert "gfx950" in device["arch"]
    assert device["cus"] >= 250


@pytest.mark.parametrize(
    "text,value",
    [("128", 128.0), ("2036Gi", 2036 * 2.0**30), ("500m", 0.5), ("288G", 288e9), (None, None)],
)
def test_quantity_to_float(text, value):
    got = bench.quantity_to_float(text)
    assert (got != got) if value is None else (got == value)
