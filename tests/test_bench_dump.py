"""bench.py --dump-outputs on the CPU: the sample of the grid path's outputs, read through a stand-in for the extractor whose device
memory is host arrays -- every read must stay inside the buffer it starts in, the sample is fixed by its seed, records and indices agree,
and what is written is finite float32 / float64 within the budget (NaN normals as 0 + a mask).  The GPU form is tests/test_bench_modes.py::test_dump_outputs_*."""
import importlib.util
import os

import numpy as np
import pytest

from volumetricterrain_amd import TRI_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    saved = dict(os.environ)   # bench.py sets its OpenMP defaults at import: they must not leak into the rest of the session
    try:
        spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.environ.clear()
        os.environ.update(saved)
    return mod


class FakeExtractor:
    """device_results() / copy_to_host() / copy_u32() over host buffers at made-up device addresses."""

    def __init__(self, tris, boffs, vc):
        self.bufs = {base: np.ascontiguousarray(a).reshape(-1).view(np.uint8) for base, a in ((0x10000000, tris), (0x20000000, boffs), (0x30000000, vc))}
        self.reads = 0

    def device_results(self):
        return 0x10000000, 0x20000000, 0x30000000

    def copy_to_host(self, d_ptr, nbytes, stream=None):
        base = max(b for b in self.bufs if b <= d_ptr)
        buf = self.bufs[base]
        assert 0 < nbytes and d_ptr + nbytes <= base + len(buf), "read outside the device buffer"
        self.reads += 1
        return buf[d_ptr - base:d_ptr - base + nbytes].copy()

    def copy_u32(self, d_ptr, count, stream=None):
        return self.copy_to_host(d_ptr, 4 * int(count), stream).view(np.uint32)


def make_outputs(n_volumes, bpv, T, seed=0):
    rng = np.random.default_rng(seed)
    per_block = rng.multinomial(T, np.ones(n_volumes * bpv) / (n_volumes * bpv))
    boffs = np.concatenate([[0], np.cumsum(per_block)]).astype(np.uint32)
    vc = np.zeros((n_volumes, 2), np.uint32)
    vc[:, 1] = per_block.reshape(n_volumes, bpv).sum(axis=1)
    vc[:, 0] = 2 * vc[:, 1]
    tris = np.zeros(T, TRI_DTYPE)
    for f in ("p0", "p1", "p2", "n0", "n1", "n2"):
        tris[f] = rng.random((T, 3), dtype=np.float32) * 8
    tris["n1"][::97] = np.nan    # a zero gradient's normal, as the device emits it
    tris["block"] = np.repeat(np.arange(n_volumes * bpv), per_block)
    return tris, boffs, vc


def check_records(out, tris, boffs):
    idx = out["triangle_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < len(tris)
    want = tris[idx]
    assert np.array_equal(out["triangle_positions"], np.stack([want["p0"], want["p1"], want["p2"]], axis=1))
    nrm = np.stack([want["n0"], want["n1"], want["n2"]], axis=1)
    assert np.array_equal(out["triangle_normals_nan"], np.isnan(nrm).astype(np.float32))     # where the library's normal was NaN ...
    assert np.array_equal(out["triangle_normals"], np.where(np.isnan(nrm), 0, nrm))            # ... written as 0: every value finite
    assert all(np.isfinite(a).all() for a in out.values())
    assert np.array_equal(out["triangle_blocks"], want["block"].astype(np.float64))
    b = want["block"]
    assert np.all(boffs[b] <= idx) and np.all(idx < boffs[b + 1])


def test_small_outputs_are_dumped_whole(bench, tmp_path):
    tris, boffs, vc = make_outputs(3, 64, 5000)
    out = bench.grid_outputs(FakeExtractor(tris, boffs, vc), 5000, 3, 64)
    assert out["triangle_count"].tolist() == [5000.0]
    assert np.array_equal(out["volume_counts"], vc.astype(np.float64)) and np.array_equal(out["block_tri_offsets"], boffs.astype(np.float64))
    assert "block_tri_offsets_index" not in out and "chunk_offsets" not in out
    assert np.array_equal(out["triangle_index"], np.arange(5000.0))
    check_records(out, tris, boffs)
    bench.write_outputs(str(tmp_path), out)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(k + ".npy" for k in out)
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all() and np.array_equal(a, out[f[:-4]])


def test_large_outputs_are_a_fixed_seeded_sample_in_bounds(bench, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_TRIANGLES", 8 * 1024)
    monkeypatch.setattr(bench, "DUMP_OFFSETS", 20000)
    T = 100000 + 77    # not a whole number of runs: the last partial run is never drawn, no read passes T
    tris, boffs, vc = make_outputs(8, 4096, T)
    ex = FakeExtractor(tris, boffs, vc)
    out = bench.grid_outputs(ex, T, 8, 4096)
    assert len(out["triangle_index"]) == 8 * 1024 and ex.reads <= 8 + 2     # eight runs of 1024 records, one copy each (adjacent runs merge) + counts + offsets
    check_records(out, tris, boffs)
    bidx = out["block_tri_offsets_index"].astype(np.int64)
    assert len(bidx) == 2 * 4096 and np.all(bidx < len(boffs))             # 32769 > 20000 entries: sampled, half the budget with its indices
    assert np.array_equal(out["block_tri_offsets"], boffs[bidx].astype(np.float64))
    again = bench.grid_outputs(FakeExtractor(tris, boffs, vc), T, 8, 4096)
    assert out["triangle_normals_nan"].any() and all(np.array_equal(out[k], again[k]) for k in out)   # NaN normals in the sample; the seed fixes it
    # at N > 1 a rank keeps its share, and the global offsets travel too
    offs = np.cumsum(np.vstack([[0, 0], vc]), axis=0)
    o2 = bench.grid_outputs(FakeExtractor(tris, boffs, vc), T, 8, 4096, offs=offs, world=2)
    assert len(o2["triangle_index"]) == 4 * 1024 and np.array_equal(o2["chunk_offsets"], offs.astype(np.float64))
    check_records(o2, tris, boffs)


def test_a_context_that_did_not_compute_this_step_is_refused(bench):
    tris, boffs, vc = make_outputs(2, 64, 1000)
    with pytest.raises(AssertionError):
        bench.grid_outputs(FakeExtractor(tris, boffs, vc), 999, 2, 64)


def test_write_outputs_enforces_dtype_budget_and_rank_names(bench, tmp_path, monkeypatch):
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "i"), {"ids": np.arange(4, dtype=np.int64)})
    for bad in (np.nan, np.inf):
        with pytest.raises(AssertionError):
            bench.write_outputs(str(tmp_path / "nf"), {"x": np.array([1.0, bad], np.float32)})
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4096)
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(1024, np.float32)})
    bench.write_outputs(str(tmp_path / "r"), {"x": np.zeros(16, np.float32)}, rank=1, world=2)
    assert os.listdir(tmp_path / "r") == ["x_rank1.npy"]
    assert not any(os.path.exists(tmp_path / d) for d in ("i", "big", "nf"))


def test_dump_outputs_is_an_argument_and_steps_sets_the_timed_steps(bench, tmp_path):
    a = bench.parse(["--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / "d")])
    assert a.steps == 7 and a.warmup == 2 and a.dump_outputs == str(tmp_path / "d")
    assert bench.parse(["--config", "stream2048", "--steps", "2"]).steps == 2
    assert bench.parse([]).dump_outputs is None
