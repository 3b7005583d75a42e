"""bench.py --dump-outputs on CPU: the sample of rows is fixed from run to run, float32, holds the tensors' own rows, and
stays within 64 MB at the bench's shapes (tests/test_gpu_bench_contract.py runs the option on the GPU)."""
import numpy as np
import torch

import bench


def _bench_outputs():
    w = bench.WORKLOAD
    B, Hq, Hkv, N, D = (w[x] for x in ("B", "Hq", "Hkv", "N", "D"))
    return {"o": torch.empty(B, Hq, N, D, device="meta"), "dq": torch.empty(B, Hq, N, D, device="meta"),
            "dk": torch.empty(B, Hkv, N, D, device="meta"), "dv": torch.empty(B, Hkv, N, D, device="meta")}


def test_dump_outputs_writes_float32_rows_reproducibly(tmp_path):
    g = torch.Generator().manual_seed(0)
    outs = {"o": torch.randn(2, 4, 64, 16, generator=g).bfloat16(), "dk": torch.randn(2, 1, 64, 16, generator=g).bfloat16()}
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    rows = bench.dump_rows(outs)
    for name, t in outs.items():
        a = np.load(tmp_path / "a" / f"{name}.npy")
        b = np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
        assert len(rows[name]) == t.numel() // 16        # small outputs are written whole
        assert np.array_equal(a, t.reshape(-1, 16).float().numpy()[rows[name]])


def test_dump_rows_at_bench_shape():
    outs = _bench_outputs()
    rows = bench.dump_rows(outs)
    D = bench.WORKLOAD["D"]
    assert set(rows) == set(outs)
    assert 32 << 20 <= sum(len(i) for i in rows.values()) * D * 4 <= 64 * 10**6
    for name, idx in rows.items():
        n_rows = outs[name].numel() // D
        assert 0 < len(idx) < n_rows and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < n_rows
    assert np.array_equal(rows["o"], rows["dq"]) and np.array_equal(rows["dk"], rows["dv"])
    again = bench.dump_rows(_bench_outputs())
    assert all(np.array_equal(rows[n], again[n]) for n in rows)
