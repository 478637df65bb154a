"""Data-parallel SAGE training, the parts that need no GPU: the seed partition against torch's DistributedSampler, the bucket layout, the
launch command and the checks the CLI makes before it touches a device."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import ddp_cases as cases


def test_partition_is_the_distributed_sampler():
    """parallel.partition(node_idx, ...) == node_idx[list(DistributedSampler(range(n), ...))] after set_epoch, element for element."""
    from graphpope_amd import parallel
    for n in cases.PARTITION_N:
        node_idx = torch.arange(n, dtype=torch.int64) * 7 + 3
        for world in cases.PARTITION_WORLD:
            sizes = set()
            for rank in range(world):
                for shuffle in (False, True):
                    for seed, epoch in ((42, 0), (42, 5), (7, 1)):
                        want = node_idx[torch.as_tensor(cases.sampler_indices(n, world, rank, shuffle, seed, epoch), dtype=torch.int64)]
                        got = parallel.partition(node_idx, world, rank, shuffle, seed, epoch)
                        assert got.dtype == torch.int64 and torch.equal(got, want), (n, world, rank, shuffle, seed, epoch)
                        sizes.add(got.numel())
            assert sizes == {-(-n // world)}                                  # every rank gets equally many: the same tail batch
    with pytest.raises(ValueError):
        parallel.partition(torch.arange(4), 2, 2, False, 0, 0)
    assert parallel.partition(torch.arange(0), 3, 1, True, 0, 0).numel() == 0


def test_partition_eval_is_a_disjoint_cover():
    from graphpope_amd import parallel
    for n in (0, 1, 2, 5, 31, 1551):
        node_idx = torch.randperm(5 * n + 1, generator=torch.Generator().manual_seed(n))[:n]
        for world in cases.PARTITION_WORLD:
            parts = [parallel.partition_eval(node_idx, world, r) for r in range(world)]
            assert sum(p.numel() for p in parts) == n                         # no padding: every node counted once
            assert sorted(torch.cat(parts).tolist()) == sorted(node_idx.tolist())
            assert max(p.numel() for p in parts) - min(p.numel() for p in parts) <= 1
    with pytest.raises(ValueError):
        parallel.partition_eval(torch.arange(4), 2, -1)


def test_grad_bucket_layout():
    """sage_grad_bucket_layout: offsets multiples of 4, increasing, non-overlapping, list order; total = the NumPy restatement; offsets
    may be NULL; a negative size or a null list is -1.  Host only."""
    from graphpope_amd import _lib, parallel
    lib = _lib.load()
    for numel in cases.LAYOUT_LISTS:
        n = len(numel)
        nn = (ctypes.c_int64 * n)(*numel)
        off = (ctypes.c_int64 * n)(*([-7] * n))
        total = lib.sage_grad_bucket_layout(n, nn, off)
        want_off, want_total = cases.layout_restatement(numel)
        assert total == want_total and list(off) == want_off, numel
        assert total % 4 == 0 and all(o % 4 == 0 for o in off)
        assert all(off[t] + numel[t] <= (off[t + 1] if t + 1 < n else total) for t in range(n))
        assert total - sum(numel) <= 3 * n
        assert lib.sage_grad_bucket_layout(n, nn, None) == total              # offsets may be NULL
        assert parallel.bucket_layout(numel) == (want_off, want_total)
    bad = (ctypes.c_int64 * 3)(4, -1, 4)
    assert lib.sage_grad_bucket_layout(3, bad, None) == -1 and lib.sage_grad_bucket_layout(2, None, None) == -1
    assert lib.sage_grad_bucket_layout(-1, bad, None) == -1
    huge = (ctypes.c_int64 * 2)(2 ** 62, 2 ** 62)
    assert lib.sage_grad_bucket_layout(2, huge, None) == -1                  # the total does not fit
    with pytest.raises(ValueError):
        parallel.bucket_layout([4, -1])
    assert lib.sage_grad_bucket_chunk() > 0 and lib.sage_grad_bucket_chunk() % 4 == 0 and lib.sage_grad_bucket_table() >= 1


def test_grad_bucket_pack_refuses_bad_arguments_without_a_gpu():
    from graphpope_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(0)
    nn = (ctypes.c_int64 * 2)(4, 4)
    some = (ctypes.c_void_p * 2)(4096, 8192)
    assert lib.sage_grad_bucket_pack(2, some, nn, 1.0, null, 8, null) == _lib.ERR_INVALID and b"flat" in lib.pope_last_error()
    assert lib.sage_grad_bucket_pack(2, some, nn, 1.0, ctypes.c_void_p(4096), 7, null) == _lib.ERR_INVALID
    assert lib.sage_grad_bucket_pack(2, null, nn, 1.0, ctypes.c_void_p(4096), 8, null) == _lib.ERR_INVALID
    hole = (ctypes.c_void_p * 2)(4096, 0)
    assert lib.sage_grad_bucket_pack(2, hole, nn, 1.0, ctypes.c_void_p(4096), 8, null) == _lib.ERR_INVALID
    assert b"tensor 1" in lib.pope_last_error()
    buf = ctypes.create_string_buffer(64)
    _lib.check(lib.pope_level_kernel_name(4096, 200, buf, 64))               # (clears the error string)
    assert lib.pope_last_error() == b""


def test_ddp_launch_command():
    from graphpope_amd import main as cli
    argv = ["--n_gpus", "2", "--dataset", "pubmed", "--epochs", "2"]
    assert cli.ddp_launch_command(argv, 2) == [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nnodes=1",
                                               "--nproc-per-node", "2", "-m", "graphpope_amd.main"] + argv
    assert cli.ddp_launch_command([], 8)[6] == "8"


def test_world_size_must_agree_with_n_gpus(monkeypatch):
    """WORLD_SIZE set: the process is one rank of that many, and --n_gpus must say so -- a ValueError before a GPU is needed (this test
    runs without one)."""
    from graphpope_amd import main as cli
    monkeypatch.setenv("WORLD_SIZE", "3")
    with pytest.raises(ValueError, match="WORLD_SIZE=3"):
        cli.main(["--n_gpus", "2", "--dataset", "pubmed", "--epochs", "1"])
    with pytest.raises(ValueError, match="WORLD_SIZE=3"):
        cli.main(["--dataset", "pubmed", "--epochs", "1"])                    # --n_gpus 1 under three ranks: the old silent trap
    assert cli.ddp_world(2, {}) == -1 and cli.ddp_world(1, {}) == 0 and cli.ddp_world(2, {"WORLD_SIZE": "2"}) == 2
    assert cli.ddp_world(1, {"WORLD_SIZE": "1"}) == 0


def test_nccl_needs_a_device_per_rank():
    from graphpope_amd import main as cli
    with pytest.raises(RuntimeError, match="gloo"):
        cli.ddp_device_index("nccl", 2, 1, 1)
    assert cli.ddp_device_index("gloo", 2, 1, 1) == 0 and cli.ddp_device_index("gloo", 3, 2, 2) == 0
    assert cli.ddp_device_index("nccl", 2, 1, 2) == 1 and cli.ddp_device_index("nccl", 2, 1, 8) == 1
    with pytest.raises(RuntimeError):
        cli.ddp_device_index("gloo", 2, 0, 0)
    assert cli.ddp_backend_from_env({}) == "nccl" and cli.ddp_backend_from_env({"GRAPHPOPE_DDP_BACKEND": "gloo"}) == "gloo"
    with pytest.raises(ValueError):
        cli.ddp_backend_from_env({"GRAPHPOPE_DDP_BACKEND": "mpi"})


def test_pack_restatement_pads_with_positive_zero():
    """The restatement the GPU test compares against: tensors at the layout's offsets, one float32 product, padding bits 0."""
    grads = [np.array([-0.0, 3.0, np.inf], dtype=np.float32), np.zeros(0, dtype=np.float32), np.array([1.0], dtype=np.float32)]
    bits = cases.pack_expected(grads, 0.5)
    assert bits.tolist() == [0x80000000, 0x3FC00000, 0x7F800000, 0, 0x3F000000, 0, 0, 0]
