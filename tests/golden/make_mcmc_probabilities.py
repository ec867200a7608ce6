"""Extracts tests/golden/mcmc_probabilities.npz from the reference's stored Bayesian run, data/mcmc_obj.rda: the recorded
results @cnv_probabilities (one 6 x 9 matrix: per region the mean of its theta samples) and @cell_probabilities (nine
6 x 10 tables: per cell the state frequencies of its 6 000 kept eps samples, multiples of 1 / 6 000).  Numbers only; the
regions they belong to are in mcmc_cell_gene.npz, in the same order.

    python tests/golden/make_mcmc_probabilities.py <checkout of the reference>"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import rda  # noqa: E402


def main(ref):
    mc = rda.read_rda(os.path.join(ref, "data", "mcmc_obj.rda"))["mcmc_obj"]
    cnv = mc.attrs["cnv_probabilities"]
    assert len(cnv) == 1
    theta_means = rda.as_matrix(cnv[0])
    cells = np.stack([rda.as_matrix(e) for e in mc.attrs["cell_probabilities"]])
    assert theta_means.shape == (6, 9) and cells.shape == (9, 6, 10)
    counts = cells * 6000.0
    assert np.abs(counts - np.rint(counts)).max() < 1e-9 and np.allclose(cells.sum(axis=1), 1.0)
    np.savez_compressed(os.path.join(HERE, "mcmc_probabilities.npz"), theta_means=theta_means, cell_probabilities=cells)
    print("theta means", theta_means.shape, "cell tables", cells.shape)


if __name__ == "__main__":
    main(sys.argv[1])
