"""GPU: posterior_patterns and ensemble_distances on ensembles with a planted answer.  All models share one cell
geometry and zeta_m = z0 + s_m q, so on any lattice the centred value matrix is s_m - mean(s) times the rasterised q:
rank one.  The leading pattern must then explain everything, correlate perfectly with every node, the distances must
be |s_a - s_b| times one constant, and chains drawn from disjoint ranges of s must show as unmixed in model space."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCELLS = 60


@pytest.fixture(scope="module")
def sds(tt):
    return tt.synthetic_rays(24, seed=1)


@pytest.fixture(scope="module")
def lattice(tt):
    xmin, xmax, ymin, ymax, zmin, zmax = tt.box()
    return np.linspace(xmin, xmax, 9), np.linspace(ymin, ymax, 7), np.linspace(zmin, zmax, 6)


@pytest.fixture(scope="module")
def planted(tt):
    """(the shared geometry, z0, q, make(s) -> Models)"""
    g = tt.random_model(NCELLS, 5)
    rng = np.random.default_rng(6)
    z0, q = rng.uniform(10.0, 40.0, NCELLS), rng.uniform(0.5, 2.0, NCELLS) * rng.choice([-1.0, 1.0], NCELLS)

    def make(s):
        return [tt.Model(float(NCELLS), g.xCell.copy(), g.yCell.copy(), g.zCell.copy(), z0 + float(sm) * q) for sm in s]

    return g, z0, q, make


@pytest.fixture(scope="module")
def two_chains(planted):
    rng = np.random.default_rng(8)
    s = [rng.uniform(-2.0, -0.5, 20), rng.uniform(0.5, 2.0, 20)]
    make = planted[3]
    return s, [make(s[0]), make(s[1])]


def rasterised_q(tt, sds, planted, lattice):
    g, _, q, _ = planted
    xs, ys, zs = lattice
    one = [tt.Model(float(NCELLS), g.xCell, g.yCell, g.zCell, q)]
    return tt.posterior_volume(one, sds, tt.define_TDstructrure(), probs=(), xs=xs, ys=ys, zs=zs)["mean"]


def test_a_rank_one_ensemble_has_one_pattern(tt, sds, planted, lattice, two_chains):
    s, nested = two_chains
    xs, ys, zs = lattice
    prm = tt.define_TDstructrure()
    out = tt.posterior_patterns(nested, sds, prm, k=3, xs=xs, ys=ys, zs=zs)
    M = 40
    assert out["scores"].shape == (M, 3) and out["patterns"].shape == (3, 9, 7, 6) and out["corr"].shape == (3, 9, 7, 6)
    print("explained", out["explained"], "participation", out["participation"])
    # rounding contributes about np u ~ 1e-13; the cap only keeps a wrong decomposition from passing
    assert out["explained"][0] >= 1 - 1e-9 and abs(out["participation"] - 1) <= 1e-9
    Q = rasterised_q(tt, sds, planted, lattice)
    assert np.all(Q != 0) and len(np.unique(Q)) > 10  # (q is nowhere 0: every node varies over the samples)
    assert np.all(out["std"] > 0) and np.all(np.abs(np.abs(out["corr"][0]) - 1) <= 1e-9)
    # the score is the centred s up to a factor and the sign rule; the pattern is q per sigma of it
    sall = np.concatenate(s)
    c = sall - sall.mean()
    sign = 1.0 if c[int(np.argmax(np.abs(c)))] > 0 else -1.0
    sc = out["scores"][:, 0]
    assert sc[int(np.argmax(np.abs(sc)))] > 0
    assert np.allclose(sc / np.linalg.norm(sc), sign * c / np.linalg.norm(c), rtol=0, atol=1e-9)
    assert np.allclose(out["patterns"][0], sign * Q * np.std(sall, ddof=1), rtol=1e-9, atol=0)
    # the maps are the existing covariance call's, bit for bit
    cov = tt.posterior_covariance(nested, sds, prm, None, series=out["scores"], xs=xs, ys=ys, zs=zs)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = cov["cov"] / cov["target_std"][:, None, None, None]
    assert np.array_equal(out["patterns"], want, equal_nan=True) and np.array_equal(out["corr"], cov["corr"], equal_nan=True)
    assert np.array_equal(out["score_std"], cov["target_std"])
    # model-space mixing in k numbers: the chains sample disjoint ranges of s, and only the first score knows
    assert out["rhat"].shape == (3,) and out["chain_of"].tolist() == [0] * 20 + [1] * 20
    print("rhat", out["rhat"], "ess", out["ess"])
    assert int(np.nanargmax(out["rhat"])) == 0 and out["rhat"][0] > 2
    # thinning keeps every second sample of each chain
    thin = tt.posterior_patterns(nested, sds, prm, k=1, thin=2, xs=xs, ys=ys, zs=zs)
    assert thin["scores"].shape == (20, 1) and thin["chain_of"].tolist() == [0] * 10 + [1] * 10 and thin["explained"][0] >= 1 - 1e-9
    with pytest.raises(ValueError, match="thin must be >= 1"):
        tt.posterior_patterns(nested, sds, prm, thin=0, xs=xs, ys=ys, zs=zs)


def test_distances_between_chains_and_the_medoid(tt, sds, planted, lattice, two_chains):
    s, nested = two_chains
    xs, ys, zs = lattice
    prm = tt.define_TDstructrure()
    out = tt.ensemble_distances(nested, sds, prm, xs=xs, ys=ys, zs=zs)
    sall = np.concatenate(s)
    gap = np.abs(sall[:, None] - sall[None, :])
    # dist = |s_a - s_b| sqrt(sum w Q^2 / W): one constant for every pair
    Q = rasterised_q(tt, sds, planted, lattice)
    w = tt.voxel_weights(xs, ys, zs)
    scale = np.sqrt(np.sum(w * Q * Q) / np.sum(w))
    assert np.isclose(out["weight_sum"], w.sum(), rtol=1e-13)
    assert np.allclose(out["dist"], gap * scale, rtol=1e-9, atol=1e-12) and np.all(np.diag(out["dist"]) == 0)
    assert np.array_equal(out["dist"], out["dist"].T)
    cd = out["chain_distance"]
    print("chain_distance", cd)
    assert cd.shape == (2, 2) and cd[0][1] == cd[1][0] and cd[0][1] > 2 * cd[0][0] and cd[0][1] > 2 * cd[1][1]
    assert out["chain_of"].tolist() == [0] * 20 + [1] * 20
    assert np.allclose(out["row_mean"], gap.sum(axis=1) * scale / 39, rtol=1e-9)
    # unweighted: every node counts 1
    plain = tt.ensemble_distances(nested, sds, prm, weights=None, xs=xs, ys=ys, zs=zs)
    assert plain["weight_sum"] == float(Q.size) and np.allclose(plain["dist"], gap * np.sqrt(np.mean(Q * Q)), rtol=1e-9, atol=1e-12)
    # a symmetric ensemble of 21: the medoid is the sample whose s is nearest the mean (the median one)
    rng = np.random.default_rng(9)
    a = rng.uniform(0.2, 2.0, 10)
    sym = np.concatenate((-a, [0.01], a))
    sym = sym[rng.permutation(21)]
    one = tt.ensemble_distances(planted[3](sym), sds, prm, xs=xs, ys=ys, zs=zs)
    assert one["medoid"] == int(np.argmin(np.abs(sym - sym.mean()))) == int(np.flatnonzero(sym == 0.01)[0])
    assert one["chain_distance"].shape == (1, 1) and one["chain_of"].tolist() == [0] * 21
