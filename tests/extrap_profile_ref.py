"""numpy reference of the extrapolation model's attention profile: a float64 group-by over the hops of tests/extrap_ref.walk.

An edge of hop l of query b with relation rel and day `day` falls into the cell (b, l, bin, rel), bin = the number of lag edges <= lag,
lag = cur_t[b] - day (the day of a self-loop is the window's first day: what the forward gives it)."""
import numpy as np


def profile_cells(hops, cur_t, B, n_rows, lag_edges):
    """(count int64 [B, L, n_bins, n_rows], alpha_sum float64 [B, L, n_bins, n_rows]) with n_bins = len(lag_edges) + 1; hops as
    extrap_ref.walk returns them: per hop (edges int64 [E, 5] = (query, head, rel, tail, data row), alpha float64 [E], day int64 [E])."""
    edges_of_bins = np.asarray(lag_edges, dtype=np.int64)
    L, n_bins = len(hops), len(edges_of_bins) + 1
    count = np.zeros((B, L, n_bins, n_rows), np.int64)
    asum = np.zeros((B, L, n_bins, n_rows), np.float64)
    cur_t = np.asarray(cur_t, dtype=np.int64)
    for l, (e, alpha, day) in enumerate(hops):
        lag = cur_t[e[:, 0]] - np.asarray(day, dtype=np.int64)
        assert (lag >= 0).all()
        b = np.searchsorted(edges_of_bins, lag, side="right")
        np.add.at(count[:, l], (e[:, 0], b, e[:, 2]), 1)
        np.add.at(asum[:, l], (e[:, 0], b, e[:, 2]), np.asarray(alpha, dtype=np.float64))
    return count, asum
