"""Generator of tests/golden/ivf_family_baseline.npz: what the IVF family answered, beyond the two plain searches that
make_pq_search_baseline.py records, at the commit before the IVF-Flat and IVF-PQ host code moved into csrc/ivf_core.h.
Three blocks per metric, on the inputs of make_pq_search_baseline.inputs("ivfpq") (N = 2000 in two adds with given ids,
NQ = 8, NLIST = 16, D = 64, M = 8):

  flat_*    FaissIvfFlat.load over x[:NLIST]: both SEARCHES with their probes, then list_sizes() and assignment()
  ht_*      the ivfpq index of build(), adopted by polysemous_ann.adopt: search(q, 10, 4, HT), last_query_codes(),
            last_ht_stats() (and the rows scanned, which the filter is measured against)
  refine_*  FaissRefineFlat.wrap over an empty ivfpq index, k_factor = 4: search(q, 10, 4) and last_candidates()

tests/test_ivf_gpu.py, tests/test_polysemous_gpu.py and tests/test_refine_gpu.py each recompute one block and ask for
byte-equal arrays.  HT was picked on the card (--choose-ht): of the even thresholds, 6, 8 and 10 are those at which the filter
bites for every metric -- 0 < rows_scored < rows_scanned, some query answers fewer than k rows and some query answers at
least one -- and 10 is the nearest to 26, where a search over 64-bit codes would start (the codebooks here are random, not
polysemous, so at 26 every query still fills its k).  The generator checks the condition and refuses to write otherwise.

usage (on a card, at the baseline commit): python tests/golden/make_ivf_family_baseline.py [dest_dir] [--ht N | --choose-ht]
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_pq_search_baseline", os.path.join(HERE, "make_pq_search_baseline.py"))
_base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_base)
inputs, build, METRICS, SEARCHES = _base.inputs, _base.build, _base.METRICS, _base.SEARCHES

HT = 10
HT_K, HT_NPROBE = 10, 4
REFINE_K, REFINE_NPROBE, REFINE_K_FACTOR = 10, 4, 4


def _metric(pkg, name):
    return getattr(pkg.dense_ann.DistanceMetric, name)


def flat_answers(pkg):
    out = {}
    x, ids, q, cent, _ = inputs("ivfpq")
    for metric in METRICS:
        ix = pkg.ivf_ann.FaissIvfFlat.load(_metric(pkg, metric), cent)
        ix.add(x[:1200], ids[:1200])
        ix.add(x[1200:], ids[1200:])
        for k, nprobe in SEARCHES:
            got_ids, dist, cnt = ix.search(q, k, nprobe)
            out[f"flat_{metric}_{k}_{nprobe}_ids"] = got_ids
            out[f"flat_{metric}_{k}_{nprobe}_dist"] = dist
            out[f"flat_{metric}_{k}_{nprobe}_cnt"] = cnt
            out[f"flat_{metric}_{k}_{nprobe}_probes"] = ix.last_probes()
        out[f"flat_{metric}_list_sizes"] = ix.list_sizes()
        out[f"flat_{metric}_assign_ids"], out[f"flat_{metric}_assign_cells"] = ix.assignment()
        ix.close()
    return out


def ht_answers(pkg, ht=HT):
    out = {}
    for metric in METRICS:
        plain, q = build(pkg, "ivfpq", metric)
        ix = pkg.polysemous_ann.adopt(plain)
        got_ids, dist, cnt = ix.search(q, HT_K, HT_NPROBE, ht)
        out[f"ht_{metric}_ids"] = got_ids
        out[f"ht_{metric}_dist"] = dist
        out[f"ht_{metric}_cnt"] = cnt
        out[f"ht_{metric}_qcodes"] = ix.last_query_codes()
        out[f"ht_{metric}_rows_scored"] = np.array([ix.last_ht_stats()["rows_scored"]], np.int64)
        out[f"ht_{metric}_rows_scanned"] = np.array([ix.last_stats()["rows_scanned"]], np.int64)
        ix.close()
    out["ht_threshold"] = np.array([ht], np.int32)
    return out


def filter_bites(block):
    """True if, for every metric, the recorded filtered search both dropped and kept rows."""
    for metric in METRICS:
        scored, scanned = int(block[f"ht_{metric}_rows_scored"][0]), int(block[f"ht_{metric}_rows_scanned"][0])
        cnt = block[f"ht_{metric}_cnt"]
        if not (0 < scored < scanned and (cnt < HT_K).any() and (cnt > 0).any()):
            return False
    return True


def refine_answers(pkg):
    out = {}
    x, ids, q, cent, cb = inputs("ivfpq")
    for metric in METRICS:
        base = pkg.ivfpq_ann.FaissIvfPq.load(_metric(pkg, metric), cent, cb)
        ix = pkg.refine_ann.FaissRefineFlat.wrap(base, k_factor=REFINE_K_FACTOR)
        ix.add(x[:1200], ids[:1200])
        ix.add(x[1200:], ids[1200:])
        got_ids, dist, cnt = ix.search(q, REFINE_K, REFINE_NPROBE)
        out[f"refine_{metric}_ids"] = got_ids
        out[f"refine_{metric}_dist"] = dist
        out[f"refine_{metric}_cnt"] = cnt
        out[f"refine_{metric}_cand_pos"], out[f"refine_{metric}_cand_cnt"] = ix.last_candidates()
        ix.close()
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from _pkg import load_package

    package = load_package()
    args = sys.argv[1:]
    if "--choose-ht" in args:  # every threshold at which the filter bites, nearest 26 first
        good = [t for t in range(2, 64, 2) if filter_bites(ht_answers(package, t))]
        print("thresholds at which the filter bites:", sorted(good, key=lambda t: (abs(t - 26), t)))
        sys.exit(0)
    ht_ = HT
    if "--ht" in args:
        at = args.index("--ht")
        ht_ = int(args[at + 1])
        del args[at:at + 2]
    dest = args[0] if args else HERE
    block = ht_answers(package, ht_)
    for metric_ in METRICS:
        print(metric_, "ht", ht_, "rows_scored", int(block[f"ht_{metric_}_rows_scored"][0]), "rows_scanned",
              int(block[f"ht_{metric_}_rows_scanned"][0]), "counts", block[f"ht_{metric_}_cnt"].tolist())
    assert filter_bites(block), f"ht = {ht_}: the filter does not bite for every metric; nothing written"
    everything = {**flat_answers(package), **block, **refine_answers(package)}
    path = os.path.join(dest, "ivf_family_baseline.npz")
    np.savez_compressed(path, **everything)
    print("wrote", path, os.path.getsize(path), "bytes")
