"""NME-SC speaker clustering on the device (csrc/kernels_cluster.hip behind capi.Diar.cluster*): each stage against a float64
numpy restatement, the whole against the host path (nemotron_asr_amd.cluster) and the NeMo fixture."""
from itertools import permutations
from pathlib import Path

import numpy as np
import pytest

from nemotron_asr_amd import capi, cluster, synth

pytestmark = pytest.mark.gpu
NEMO = Path(__file__).parent / "golden" / "nemo_diar_v1.npz"


@pytest.fixture(scope="module")
def eng():
    e = capi.Diar(synth.make_diar_weights(spk=False))
    yield e
    e.close()


def _accuracy(got, ref):
    K = int(max(got.max(), ref.max())) + 1
    return max(np.mean(np.asarray(perm)[got] == ref) for perm in permutations(range(K)))


def _speakers(n_each, noise=0.35, dim=192, seed=5):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((len(n_each), dim))
    truth = np.repeat(np.arange(len(n_each)), n_each)
    return (centres[truth] + noise * rng.standard_normal((truth.size, dim))).astype(np.float32)


@pytest.mark.parametrize("case", ["nemo", "random"])
def test_affinity(eng, case):
    if case == "nemo":
        g = np.load(NEMO)
        emb, ref = g["cluster_embeddings"], g["cluster_affinity"]
    else:                                            # odd N, D not a multiple of the MFMA's K
        emb = np.random.default_rng(0).standard_normal((37, 10)).astype(np.float32)
        norm = np.sqrt((emb.astype(np.float64) ** 2).sum(1).astype(np.float32))
        unit = (emb * (np.float32(1.0) / (norm + np.float32(3.5e-4)))[:, None]).astype(np.float64)
        ref = unit @ unit.T
        np.fill_diagonal(ref, 1.0)
        ref = (ref - ref.min()) / (ref.max() - ref.min())
    aff = eng.cluster_affinity(emb)
    assert np.abs(aff - ref).max() < 2e-6
    assert aff.min() == 0.0 and aff.max() == 1.0 and (np.diag(aff) == 1.0).all() and (aff == aff.T).all()


@pytest.mark.parametrize("N,p", [(5, 1), (37, 9), (130, 130), (200, 50)])
def test_graph_keeps_the_p_largest_with_ties_by_index(eng, N, p):
    emb = np.random.default_rng(N).standard_normal((N, 16)).astype(np.float32)
    emb[N // 2] = emb[1]                             # duplicated rows: equal entries in every row of the affinity
    emb[N - 1] = emb[0]
    emb[2] = emb[1]
    aff = cluster.cosine_affinity(emb)
    keep = np.zeros((N, N), np.float32)
    for i in range(N):
        keep[i, np.argsort(-aff[i], kind="stable")[:p]] = 1.0
    assert (eng.cluster_graph(aff, p) == 0.5 * (keep + keep.T)).all()


@pytest.mark.parametrize("n", [1, 2, 3, 40, 67, 200])
def test_eigen_solver_against_numpy(eng, n):
    rng = np.random.default_rng(n)
    m = rng.standard_normal((3, n, n))
    m = (m + m.transpose(0, 2, 1)) / 2
    k = min(n, 8)
    low, top, vec = eng.sym_eigen(m, k)
    ref = np.linalg.eigvalsh(m)
    tol = 1e-11 * max(1.0, np.abs(m).max() * n)
    assert np.abs(low - ref[:, :k]).max() < tol and np.abs(top - ref[:, -1]).max() < tol
    assert np.abs(m[0] @ vec - vec * low[0]).max() < 1e-11 * n and np.abs(vec.T @ vec - np.eye(k)).max() < 1e-11 * n


def test_eigen_solver_degenerate_laplacian(eng):
    """3 disconnected 7-cliques: eigenvalue 0 three times, exact splits in the tridiagonal"""
    k, size = 3, 7
    a = np.kron(np.eye(k), np.ones((size, size)))
    np.fill_diagonal(a, 0.0)
    lap = np.diag(a.sum(1)) - a
    low, top, vec = eng.sym_eigen(lap, k + 1)
    assert np.abs(low[0, :k]).max() < 1e-12 and abs(low[0, k] - size) < 1e-10 and abs(top[0] - size) < 1e-10
    V = vec[:, :k]
    assert np.abs(lap @ V).max() < 1e-10 and np.abs(V.T @ V - np.eye(k)).max() < 1e-10


def test_nmesc_matches_nemo_labels_speaker_count_and_p(eng):
    g = np.load(NEMO)
    max_spk, volume, mat = (int(v) for v in g["cluster_meta"][2:])
    labels, est, p_hat = eng.cluster(g["cluster_embeddings"], max_spk, float(g["cluster_max_rp_threshold"]), volume, mat)
    assert (est, p_hat) == (2, 15) and _accuracy(labels, g["cluster_labels"]) == 1.0


@pytest.mark.parametrize("nme_mat_size", [512, 32])
def test_clusters_like_the_host_path(eng, nme_mat_size):
    emb = _speakers([25, 40, 18])
    ref, est_ref, p_ref = cluster.nmesc_cluster(emb, nme_mat_size=nme_mat_size)
    labels, est, p_hat = eng.cluster(emb, nme_mat_size=nme_mat_size)
    assert (est, p_hat) == (est_ref, p_ref) and est == 3 and _accuracy(labels, ref) == 1.0
    assert nme_mat_size == 512 or p_hat % 3 == 0     # subsampled analysis: p_hat = ratio (3) x p
    assert eng.last_gpu_ms("cluster") > 0.0


def test_forced_count_early_return_and_errors(eng):
    emb = _speakers([25, 40, 18])
    labels, est, _ = eng.cluster(emb, oracle_num_speakers=2)
    assert est == 2 and set(labels) == {0, 1}
    few, est_few, p_few = eng.cluster(emb[:5])
    assert (few == 0).all() and est_few == 1 and p_few == 4
    for bad in (np.zeros((0, 192), np.float32), np.zeros((capi.CLUSTER_MAX_N + 1, 4), np.float32)):
        with pytest.raises(capi.NasrError):
            eng.cluster(bad)
