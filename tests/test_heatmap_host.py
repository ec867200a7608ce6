"""Host pieces of plot_cnv (infercnv_amd/heatmap.py, DESIGN K17) that need no GPU: R's number formatting, the palettes, the
type-7 quantile formula of the restatement, cutree(k)."""
import numpy as np
import pytest

import heatmap_restate as hmr
from infercnv_amd import _lib
from infercnv_amd import heatmap as hm
from infercnv_amd.tumor_subclusters import cutree_h

FORMATS = [(100000.0, "1e+05"), (123456.0, "123456"), (0.0001, "1e-04"), (0.00012, "0.00012"), (1.0, "1"), (0.1 + 0.2, "0.3"),
           (-0.5, "-0.5"), (1234567.1, "1234567.1"), (1e15, "1e+15"), (1e-300, "1e-300"), (0.0, "0"), (1 / 3, "0.333333333333333"),
           (2.0 / 3.0 * 1e-5, "6.66666666666667e-06"), (123456789012345678.0, "123456789012346000"), (7, "7")]


@pytest.mark.parametrize("value,text", FORMATS)
def test_r_num(value, text):
    assert hm.r_num(value) == text
    assert hmr.r_num(value) == text


def test_r_num_agrees_with_restatement_on_random_values():
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.normal(1, 0.1, 300), 10.0 ** rng.uniform(-12, 18, 300) * rng.choice([-1, 1], 300),
                           np.round(rng.normal(0, 100, 100), 2), rng.integers(-10**6, 10**6, 100).astype(float)])
    for v in vals:
        s = hm.r_num(v)
        assert s == hmr.r_num(v)
        assert float(s) == float("%.15g" % v)          # the text is the 15-digit rounding, whatever the notation


def test_set3():
    brewer = ["#8DD3C7", "#FFFFB3", "#BEBADA", "#FB8072", "#80B1D3", "#FDB462", "#B3DE69", "#FCCDE5", "#D9D9D9", "#BC80BD",
              "#CCEBC5", "#FFED6F"]
    assert hm.group_colors(12) == brewer and hmr.brewer_set3(12) == brewer
    assert hm.group_colors(1) == ["#8DD3C7"] and hmr.brewer_set3(1) == ["#8DD3C7"]
    assert hm.group_colors(2) == ["#8DD3C7", "#FFED6F"]
    for n in (3, 4, 5, 22, 24):
        assert hm.group_colors(n) == hmr.brewer_set3(n) and len(hm.group_colors(n)) == n


def test_heat_palettes():
    pal = hm.color_palette(("darkblue", "white", "darkred"), (2, 2))(15)
    assert pal == hmr.color_palette(("darkblue", "white", "darkred"), (2, 2), 15)
    assert (pal[0], pal[7], pal[14]) == ("#00008B", "#FFFFFF", "#8B0000") and len(set(pal)) == 15
    safe = hm.color_palette(("purple3", "white", "darkorange2"), (2, 2))(15)
    assert safe == hmr.color_palette(("purple3", "white", "darkorange2"), (2, 2), 15)
    assert (safe[0], safe[7], safe[14]) == ("#7D26CD", "#FFFFFF", "#EE7600")


def test_type7_formula():
    x = np.arange(101, dtype=np.float64) * 0.5          # n = 101: (n - 1) p is an integer for p = 0.01, 0.99
    r = hmr.quantiles_excluding(x, np.nan, (0.01, 0.99, 0.5, 0.0, 1.0))
    assert r["quantiles"].tolist() == [0.5, 49.5, 25.0, 0.0, 50.0]
    assert r["lo"].tolist() == r["hi"].tolist() == [0.5, 49.5, 25.0, 0.0, 50.0]
    y = np.arange(100, dtype=np.float64)                # n = 100: index = 99 p
    r = hmr.quantiles_excluding(y, np.nan, (0.01, 0.99, 0.5))
    assert r["lo"].tolist() == [0.0, 98.0, 49.0] and r["hi"].tolist() == [1.0, 99.0, 50.0]
    for q, p in zip(r["quantiles"], (0.01, 0.99, 0.5)):
        index = 99.0 * p
        h = index - np.floor(index)
        assert q == (1.0 - h) * np.floor(index) + h * np.ceil(index)
    # the excluded value, both zeros as one value, and the x_(hi) == x_(lo) shortcut
    z = np.array([1.0, -0.0, 0.0, 1.0, 3.0, 1.0, 3.0])
    r = hmr.quantiles_excluding(z, 1.0, (0.3, 0.5))
    assert (r["n_kept"], r["n_excluded"]) == (4, 3) and r["quantiles"].tolist() == [0.0, 1.5]
    assert not np.signbit(r["quantiles"][0]) and not np.signbit(r["min"])


def test_cutree_k_against_cutree_h():
    import hclust_restate as hr
    X = np.random.default_rng(6).normal(size=(23, 5))
    merge, height, _ = hr.hclust(hr.seq_dist(X), "average")
    assert np.all(np.diff(height) > 0)
    n = 23
    for k in range(1, n + 1):
        h = 0.0 if k == n else (height[n - k - 1] + (height[n - k] if k > 1 else height[-1] + 1.0)) / 2   # between the merges
        want = cutree_h(merge, height, h)
        assert np.array_equal(hm.cutree_k(merge, k), want) and np.array_equal(hmr.cutree_k(merge, k), want)
        assert len(set(want.tolist())) == k
    with pytest.raises(ValueError):
        hm.cutree_k(merge, 0)


def test_prototypes_and_page_geometry():
    for name in ("icnv_quantiles_excluding_dev", "icnv_quantiles_excluding", "icnv_heatmap_bins_dev", "icnv_heatmap_bins",
                 "icnv_heatmap_raster_dev", "icnv_heatmap_raster", "icnv_heatmap_stats", "icnv_heatmap_stats_reset"):
        assert name in _lib.PROTOTYPES
    geo = hm.page_geometry(["tumor"], ["normal"], 10, 300, 0)
    assert (geo["width"], geo["height"]) == (3000, round((8.22 + 3 * 0.175 + 4 * 0.175) * 300))
    W, H, xs, ys = hmr.page_geometry(["tumor"], ["normal"], 10, 300, 0)
    assert (W, H) == (geo["width"], geo["height"])
    assert geo["panels"]["observations"] == [xs[4], ys[3], xs[14], ys[12]] and xs[14] == W
    assert ys[12] - ys[3] == 1350                       # nine layout rows of half an inch at 300 dpi
    tall = hm.page_geometry(["tumor"], [], 5000, 300, 2)
    assert tall["height"] <= 32767 and tall["height_in"] == round(32767 / 300 - 0.005, 2)
