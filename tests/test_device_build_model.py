"""CPU tests of tests/device_build_model.py, the checker of tests/test_gpu_device_build.py: the model's CSR lists and
codes against scann_rust_amd.trainer.build_txh_index on the model's own centres and assignment, the training-row rule,
and the condition the GPU freeze case rests on (the per-subspace iteration counts really differ)."""
import ctypes

import numpy as np

from oracle import pyoracle as orc
from scann_rust_amd import trainer
from tests import device_build_model as DM


def seeds_for(rows, cfg):
    dsub = rows.shape[1] // cfg["num_subspaces"]
    return (lambda k: DM.stream_seeds(rows, k, 42),
            lambda train, s, kc: DM.stream_seeds(train[:, s * dsub:(s + 1) * dsub], kc, 42 + s))


def run(name):
    rows, stride, cfg = DM.case(name)
    st = int(orc.compute_stride(rows.shape[1])) if stride is None else stride
    return rows, cfg, DM.model(rows, st, cfg, *seeds_for(rows, cfg))


def test_csr_and_codes_match_the_trainer():
    rows, cfg, m = run("tree")
    t = trainer.build_txh_index(rows, cfg["num_partitions"], cfg["num_subspaces"], cfg["num_codes"], pq_iters=1,
                                centers=m["centers"], assign=m["leaf"])
    assert np.array_equal(t["leaf_off"], m["leaf_offsets"]) and np.array_equal(t["leaf_ids"], m["leaf_ids"])
    # ascending datapoint index inside every leaf, every row in the leaf k-means assigned it to
    for l in range(m["L"]):
        ids = m["leaf_ids"][m["leaf_offsets"][l]:m["leaf_offsets"][l + 1]]
        assert np.all(np.diff(ids.astype(np.int64)) > 0) and np.all(m["leaf"][ids] == l)
    # the codes: the trainer's statement of Codebook::encode on the residual rows in CSR order, model's codebook
    order = m["leaf_ids"]
    resid_csr = rows[order] - m["centers"][m["leaf"][order]]
    assert np.array_equal(trainer.encode(m["codebook"], resid_csr), m["codes"])
    assert np.array_equal(trainer.pack4(m["codes"]), m["codes_file"])


def test_training_rows_are_residuals_against_partition_tokens_in_datapoint_order():
    rows, cfg, m = run("partition-dim-128")
    assert np.array_equal(m["train"], rows - m["centers"][m["token"]])
    # at 128 dims the k-means assignment (AVX2 order) and partition(x, 1) (sequential) are different functions; the
    # model keeps them apart even where they agree on these rows
    tok = np.array([orc.partition(m["centers"], r, 1)[0][0] for r in rows])
    assert np.array_equal(tok, m["token"])
    _, cfg0, m0 = run("no-residuals")
    assert m0["train"] is not None and "token" not in m0 and np.array_equal(m0["train"], DM.case("no-residuals")[0])


def test_flat_and_small_cases():
    _, cfg, m = run("flat")
    assert m["L"] == 0 and np.array_equal(m["order"], np.arange(m["n"]))
    _, cfg, m = run("fewer-rows-than-codes")
    kc = m["n"]
    assert kc < cfg["num_codes"]
    assert all(np.array_equal(m["codebook"][s, kc:], np.repeat(m["codebook"][s, kc - 1:kc], cfg["num_codes"] - kc, 0))
               for s in range(cfg["num_subspaces"]))
    assert m["codes"].max() < kc          # strict '<': a repeated centre never wins
    _, cfg, m = run("more-leaves-than-rows")
    assert m["L"] == m["n"] == 5
    _, cfg, m = run("zero-iterations")
    assert m["partition_iterations"] == 0 and not m["partition_converged"] and not any(m["subspace_iterations"])


def test_freeze_case_iteration_counts_differ():
    """the condition of the GPU freeze case: under one training_iterations cap at least one subspace converges early
    and at least one runs into the cap"""
    _, cfg, m = run("freeze")
    cap = cfg["training_iterations"]
    its, conv = m["subspace_iterations"], m["subspace_converged"]
    assert any(c and i < cap for i, c in zip(its, conv)), (its, conv)
    assert any((not c) and i == cap for i, c in zip(its, conv)), (its, conv)
    assert len(set(its)) > 1


def test_ctypes_layout_of_the_build_structs():
    """hip.BuildConfig / BuildReport against the compiled library's sizeof / offsetof (scann_hip_abi_layout words 6-9)"""
    from scann_rust_amd import build, hip
    build.build()
    lay = hip.abi_layout(10)
    assert lay[:6] == hip.abi_layout()
    assert lay[6:] == [ctypes.sizeof(hip.BuildConfig), hip.BuildConfig.distance_measure.offset,
                       ctypes.sizeof(hip.BuildReport), hip.BuildReport.stage_ms.offset]
    c = hip.build_config(num_partitions=7)
    assert (c.num_partitions, c.kmeans_iterations, c.kmeans_seed, c.training_iterations, c.seed, c.simd_threshold,
            c.use_residuals, c.store_rows, c.partitions_to_search) == (7, 100, 42, 25, 42, 128, 1, 1, 10)
    assert c.kmeans_convergence == 1e-5 and c.convergence_threshold == 1e-5 and c.pre_reorder_multiplier == 3.0
