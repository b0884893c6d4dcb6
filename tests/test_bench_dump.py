"""CPU: bench.py --dump-outputs writes what the forward returned -- small arrays whole, large ones as the same
seeded sample in every run -- as float32 .npy files within its byte budget."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402


def _outputs():
    g = torch.Generator().manual_seed(0)
    st = {"depth": torch.rand(2, 5, 7, generator=g), "prob_volume": torch.rand(2, 8, 5, 7, generator=g).bfloat16(),
          "depth_values": torch.rand(2, 8, 5, 7, generator=g)}
    out = {"stage1": st, "stage2": {"depth": torch.rand(2, 10, 14, generator=g)}}
    out.update(st)  # the forward's top-level aliases of the last stage
    return out


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    out = _outputs()
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 4 * 100)  # 4 arrays, 100 elements each
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    wa, wb = bench.dump_outputs(out, a), bench.dump_outputs(out, b)
    assert wa == wb and sorted(os.listdir(a)) == sorted(n + ".npy" for n in wa)
    assert sorted(wa) == ["stage1.depth", "stage1.depth_values", "stage1.prob_volume", "stage2.depth"]
    total = 0
    for name in wa:
        x, y = np.load(os.path.join(a, name + ".npy")), np.load(os.path.join(b, name + ".npy"))
        assert x.dtype == np.float32 and np.array_equal(x, y)
        total += x.nbytes
        st, key = name.split(".")
        src = out[st][key].float().numpy()
        if src.size <= 100:
            assert np.array_equal(x, src)
        else:
            idx = np.random.default_rng(0).integers(0, src.size, 100)
            assert np.array_equal(x, src.reshape(-1)[idx])
    assert total <= 4 * 4 * 100
    assert wa["stage1.depth"] == [[2, 5, 7], 70] and wa["stage1.prob_volume"] == [[2, 8, 5, 7], 100]


def test_dump_budget_is_below_64_mb():
    assert bench.DUMP_BYTES <= 64 * 10 ** 6
