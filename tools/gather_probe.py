"""Measurement: the unit kernel's gather on its own (sann_debug_gather_probe) on the bench workload.

First the three forms of the gather -- the 16-byte postings (mode 0), the id column with one 8-byte load per posting
(mode 2) and the id column in aligned 16-byte pairs (mode 3) -- taken in turns, ROUNDS times each, so that the spread over
the repetitions is known; then the ladder of ablated unit kernels (modes 10..19).  GATHER_PROBE_LADDER=0 skips the ladder."""
import ctypes as C
import os
import statistics
import sys

os.environ.setdefault("SANN_NO_TORCH", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_package()
lib = pkg.load_library()
P = int(sys.argv[1]) if len(sys.argv) > 1 else 32
T = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
ROUNDS = int(os.environ.get("GATHER_PROBE_ROUNDS", "12"))
offs, cids, scs = pkg.corpus.make_queries(1024)
index = pkg.ClusterTweetIndex.synthetic(T, n_partitions=P)
cfg = pkg.SimClustersANNConfig(maxNumResults=400, annAlgorithm=pkg.ScoringAlgorithm.CosineSimilarity)
qb = pkg.QueryBatch(index, offs, cids, scs, cfg, now_ms=pkg.corpus.NOW_MS)
for _ in range(3):
    qb.run(); qb.finish()
st = qb.stats()
print("P", P, "postings", st.postings_scanned, "bytes", st.algorithmic_bytes, "max unit", st.max_unit_postings)
ms, cs = C.c_double(), C.c_uint64()


def probe(mode, wgs, reps):
    rc = lib.sann_debug_gather_probe(qb._h, mode, wgs, reps, C.byref(ms), C.byref(cs))
    assert rc == 0, lib.sann_last_error()
    return ms.value * 1e3


FORMS = [(0, "16-byte postings", 16), (2, "id column, 8 B per lane", 8), (3, "id column, aligned 16-B pairs", 8)]
times = {m: [] for m, _, _ in FORMS}
for _ in range(ROUNDS):
    for m, _, _ in FORMS:
        times[m].append(probe(m, 1, 5))  # (one warm-up launch, then the mean of five)
for m, name, width in FORMS:
    t = times[m]
    print(f"form {m} ({name}): median {statistics.median(t):7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}  "
          f"stdev {statistics.pstdev(t):5.2f}  over {len(t)} repetitions  "
          f"{st.postings_scanned * width / statistics.median(t) / 1e6:6.2f} TB/s of posting bytes")

if os.environ.get("GATHER_PROBE_LADDER", "1") != "0":
    for mode, wgs in [(0, 1), (1, 6), (16, 1), (17, 1), (11, 1), (12, 1), (13, 1), (14, 1), (18, 1), (19, 1), (15, 1), (10, 1)]:
        t = probe(mode, wgs, 10)
        print(f"mode {mode} wgs/cu {wgs}: {t:8.1f} us  {st.algorithmic_bytes/t/1e6:7.2f} TB/s  checksum {cs.value:016x}")
