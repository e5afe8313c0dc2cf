"""The filtered rank of include/redgnn.h (rg_rank) in numpy, counted in integers: the comparison with the kernel is exact equality.
TEST INFRASTRUCTURE.

    s'      = fl32(fl32(s - rowmin) + 1e-8)
    rank(a) = #{j not in filter: s'_j > s'_a} + (#{j: s'_j == s'_a} + 1) / 2

Answers and filters are CSR lists over the queries; a filter list is a set (no entity twice) that contains the query's answers."""
import numpy as np


def shifted(row):
    row = np.asarray(row, np.float32)
    return ((row - row.min()).astype(np.float32) + np.float32(1e-8)).astype(np.float32)


def ranks(scores, ans_ptr, ans_idx, filt_ptr, filt_idx):
    """float64 [len(ans_idx)] in (query, answer-list) order; every value is a multiple of 1/2 formed from integer counts."""
    scores = np.asarray(scores, np.float32)
    out = np.zeros(len(ans_idx), np.float64)
    for q in range(scores.shape[0]):
        s = shifted(scores[q])
        unfiltered = np.ones(len(s), bool)
        unfiltered[np.asarray(filt_idx[filt_ptr[q]:filt_ptr[q + 1]], np.int64)] = False
        for i in range(ans_ptr[q], ans_ptr[q + 1]):
            sa = s[ans_idx[i]]
            gt = int(np.count_nonzero((s > sa) & unfiltered))
            eq = int(np.count_nonzero(s == sa))
            out[i] = (2 * gt + eq + 1) / 2.0
    return out


def to_dense(n_ent, ans_ptr, ans_idx, filt_ptr, filt_idx):
    """(labels, filters) float64 [B, n_ent] of the CSR lists, as utils.cal_ranks of the reference takes them."""
    B = len(ans_ptr) - 1
    labels, filters = np.zeros((B, n_ent)), np.zeros((B, n_ent))
    for q in range(B):
        labels[q, ans_idx[ans_ptr[q]:ans_ptr[q + 1]]] = 1
        filters[q, filt_idx[filt_ptr[q]:filt_ptr[q + 1]]] = 1
    return labels, filters


def to_csr(labels, filters):
    """CSR lists of dense labels / filters, entities ascending inside a query (the order cal_ranks returns its ranks in)."""
    ap, fp = [0], [0]
    ai, fi = [], []
    for l, f in zip(np.asarray(labels), np.asarray(filters)):
        ai += np.nonzero(l)[0].tolist()
        fi += np.nonzero(f)[0].tolist()
        ap.append(len(ai))
        fp.append(len(fi))
    i32 = lambda a: np.asarray(a, np.int32)
    return i32(ap), i32(ai), i32(fp), i32(fi)


ROW_KINDS = ("no_answers_no_filter", "one_answer", "fifty_answers_long_filter", "all_equal", "mostly_zero", "negatives", "quantised")


def batch(n_ent, seed=0):
    """One batch for rg_rank at ``n_ent`` entities, a row per kind in ROW_KINDS (finite scores only):
      no answers and a filter list of length 0;  one answer (filter = that answer);  50 answers inside a filter list of 300 entries
      (longer than one 256-thread pass);  a row where all scores are equal;  a row of exact zeros with a few positives (the real shape
      of a score row: unvisited entities score 0), answers among both;  a row of negatives;  a row of heavy ties (scores rounded to one
      decimal).  Below 50 / 300 entities a filter list is the whole entity set (a filter is a set) and the 50 answers repeat entities.
    Returns (scores fp32 [7, n_ent], ans_ptr, ans_idx, filt_ptr, filt_idx int32)."""
    rng = np.random.default_rng(seed + n_ent)
    B = len(ROW_KINDS)
    scores = rng.standard_normal((B, n_ent)).astype(np.float32)
    scores[3] = np.float32(0.37)
    scores[4] = 0
    pos = rng.choice(n_ent, min(n_ent, 40), replace=False)
    scores[4, pos] = np.abs(rng.standard_normal(len(pos))).astype(np.float32) + np.float32(1e-3)
    scores[5] = -np.abs(scores[5]) - np.float32(0.5)
    scores[6] = np.round(scores[6], 1)
    ans, filt = [], []
    for q in range(B):
        if q == 0:
            a, f = np.zeros(0, np.int64), np.zeros(0, np.int64)
        elif q == 1:
            a = rng.integers(0, n_ent, 1)
            f = a.copy()
        else:
            f = np.sort(rng.choice(n_ent, min(n_ent, 300), replace=False))
            if q == 4:      # answers among the positives and among the zeros
                f = np.unique(np.concatenate([f, pos[:5]]))
            a = np.sort(rng.choice(f, 50, replace=len(f) < 50))
            if q == 4 and len(f) >= 50:
                a = np.sort(np.concatenate([pos[:5], rng.choice(np.setdiff1d(f, pos[:5]), 45, replace=False)]))
        ans.append(a)
        filt.append(f)
    ptr = lambda lists: np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    cat = lambda lists: np.concatenate(lists).astype(np.int32)
    return scores, ptr(ans), cat(ans), ptr(filt), cat(filt)
