"""bench.py host-side pieces that need no GPU: the committed PMC summary it prices HBM
traffic from exists and has the kernels the JSON line reports."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_pmc_summary_is_committed_and_covers_the_reported_kernels():
    import bench
    assert os.path.exists(os.path.join(REPO, "profiles", bench.PMC_SUMMARY))
    # the kernels of the default configuration (bench.gru_bwd_kernel / gru_fwd_kernel name them)
    for prefix, extra in (("gemm", ("splitk_reduce_kernel",)),
                          (bench.gru_bwd_kernel(True)[2], ()), (bench.gru_fwd_kernel(True)[2], ())):
        traffic, src = bench.pmc_traffic_per_launch(prefix, extra)
        assert src == os.path.join("profiles", bench.PMC_SUMMARY)
        assert traffic is not None and traffic > 1e8, prefix


def test_dump_outputs_writes_seeded_float_arrays(tmp_path, monkeypatch):
    """bench.dump_outputs: loss, scores, parameters and gradients as float32/float64 .npy; a
    flat array above DUMP_SAMPLE is sampled at the same sorted positions in every run."""
    import types
    import numpy as np
    import torch
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    loss = model(torch.randn(4, 7)).square().sum()
    loss.backward()
    tr = types.SimpleNamespace(model=model, train_wer=3.0, train_cer=11.0, num_words=8.0,
                               num_chars=40.0)
    flat_p = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    flat_g = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).numpy()

    bench.dump_outputs(str(tmp_path / "all"), tr, loss.detach())
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["grads", "loss", "params", "score"]
    assert got["loss"].dtype == np.float32 and got["loss"].tolist() == [loss.item()]
    assert got["score"].dtype == np.float64 and got["score"].tolist() == [3.0, 11.0, 8.0, 40.0]
    assert got["params"].dtype == np.float32 and np.array_equal(got["params"], flat_p)
    assert got["grads"].dtype == np.float32 and np.array_equal(got["grads"], flat_g)

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 16)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), tr, loss.detach())
    g = torch.Generator().manual_seed(bench.DUMP_SEED)
    ii = torch.randint(0, flat_p.size, (16,), generator=g).sort().values.numpy()
    assert sorted(os.listdir(tmp_path / "s1")) == ["grads.npy", "loss.npy", "params.npy",
                                                   "score.npy"]
    assert np.array_equal(np.load(tmp_path / "s1" / "params.npy"), flat_p[ii])
    assert np.array_equal(np.load(tmp_path / "s2" / "grads.npy"), flat_g[ii])


def test_bench_probes_every_recurrence_entry_point():
    """bench.py times the GRU recurrences by wrapping the C-ABI entry points ops.py calls: every
    ds2_gru_fwd* / ds2_gru_bwd* name the GRU layer calls must be one the probes wrap (a renamed
    entry point silently dropped the backward from the bench line once)."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "deepspeech.pytorch_amd", "ds2amd", "ops.py")).read()
    called = set(re.findall(r'"(ds2_gru_(?:fwd|bwd)\w*)"', src)) - {
        "ds2_gru_fwd_workspace_size", "ds2_gru_bwd_workspace_size", "ds2_gru_bwd_grid"}
    bench_src = open(os.path.join(root, "bench.py")).read()
    probed = set(re.findall(r'"(ds2_gru_(?:fwd|bwd)\w*)"', bench_src))
    assert called and called <= probed, sorted(called - probed)
