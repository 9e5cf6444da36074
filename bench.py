#!/usr/bin/env python3
"""bench.py -- candidates/sec of batched SimClusters-ANN getTweetCandidates on MI355X.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path over one batch of synthetic user queries whose prepared
form (embeddings, cluster rows, weights) and whose index are already resident in HBM:
gather posting lists -> ordered fp64 accumulate -> normalise -> filter -> exact top-k, i.e.
ApproximateCosineSimilarity.apply (reference simclusters-ann/.../candidate_source/
ApproximateCosineSimilarity.scala:57-128) for every query of the batch.

N = 1   workload = BASELINE.json configs[2]: 1024 concurrent user queries, one GPU.
N > 1   the corpus is tweet-hash sharded over the N ranks (one process per GPU); every rank
        answers the whole batch (1024*N queries) on its shard; each query has an owner rank, the
        per-shard lists (cut at k/N + 6 sigma + 8 entries) reach the owners in one RCCL all-to-all
        and the owner merges them exactly, proving the cut harmless (ComposedQueryable pattern,
        reference ann/.../common/ShardApi.scala:71-87).  Per-GPU posting work is constant in N:
        "scaling": "weak".

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps steps and prints the headline
(`value`, `ms_per_step`); --full also measures and checks everything beside it, after the timed steps: per-kernel
timings (`roofline`), the `end_to_end` and `micro_batched` legs, oracle parity, both recall fields, `cpu_baseline` and,
sharded, the comparison with the unsharded index.  --dump-outputs DIR writes what the last timed step returned.
"""
import argparse
import ctypes
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: all files together


def dump_outputs(out_dir, ids, scores, counts, map_sizes, limit_bytes=DUMP_LIMIT_BYTES):
    """--dump-outputs: the answer a caller of the timed path receives (ids, scores, counts, map sizes per query) as float64
    DIR/<name>.npy.  Tweet ids are 63-bit snowflakes, beyond float64's 53-bit mantissa: they are written as their high and
    low 32 bits.  Entries past a query's count are not part of its answer and are written as 0.  When the whole answer
    would exceed `limit_bytes`, a fixed seeded sample of query rows is written; `query_index` names the rows either way."""
    ids, scores = np.asarray(ids, np.int64), np.asarray(scores, np.float64)
    counts, map_sizes = np.asarray(counts), np.asarray(map_sizes)
    nq, k = ids.shape
    rows = np.arange(nq)
    max_rows = (limit_bytes - 6 * 4096) // ((3 * k + 3) * 8)  # (six files: a header allowance each)
    if nq > max_rows:
        rows = np.sort(np.random.default_rng(20260105).choice(nq, size=max_rows, replace=False))
    ids, scores, counts, map_sizes = ids[rows], scores[rows].copy(), counts[rows], map_sizes[rows]
    past = np.arange(k)[None, :] >= counts[:, None]
    ids = np.where(past, 0, ids)
    scores[past] = 0.0
    os.makedirs(out_dir, exist_ok=True)
    for name, a in (("query_index", rows), ("tweet_ids_hi32", ids >> 32), ("tweet_ids_lo32", ids & 0xFFFFFFFF), ("scores", scores),
                    ("counts", counts), ("map_sizes", map_sizes)):
        np.save(os.path.join(out_dir, name + ".npy"), np.asarray(a, np.float64))


def traffic_bytes(args, nq, world):
    """HBM bytes per launch of the dominant kernel from the committed PMC pass (profiles/traffic.json:
    (2 x FETCH_SIZE + WRITE_SIZE) x 1024, the gfx950 correction of MI355X_MICROARCH.md), when a
    pass for exactly this workload was committed; else None."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        return t.get(f"tweets={args.tweets},queries={nq},alg={args.alg},gpus={world},partitions={args.partitions or 32}")
    except Exception:
        return None


def run_cluster_range(args, pkg, lib, index, comm, dist, torch, rank, world, local_rank, nq, nql, qsets, cfg, K, shard_k, now_ms, json_fd, t_corpus):
    """--sharding cluster-range: rank g serves the clusters of id range g (equal id counts: at 100M tweets nearly every list is at
    the index cap, so id count = posting mass); every step runs sharding.ClusterRangeRank.step -- export, exchange of the scanned
    prefixes by tweet hash over RCCL, temporary index, ordinary batch, exchange to the owners, proving merge.  The batch's scanned
    clusters (host arithmetic over the queries) are worked out before the timed region, like the prepared batches of the
    tweet-hash path."""
    import dataclasses
    assert comm is not None, "--sharding cluster-range needs the library's RCCL communicator (backend nccl)"
    sh = pkg.sharding
    C_all = pkg.corpus.N_CLUSTERS
    first = 1 + rank * C_all // world
    end = 1 + (rank + 1) * C_all // world if rank + 1 < world else C_all + 1
    rr = sh.ClusterRangeRank(pkg, index, comm, rank, world, first, end, device=local_rank, n_partitions=args.partitions)
    cfg_run = cfg if shard_k == K else dataclasses.replace(cfg, maxNumResults=shard_k)
    needs = [sh.scanned_clusters(o, c, s, int(cfg.maxScanClusters)) for (o, c, s) in qsets]
    out_ids = torch.zeros((nql, K), dtype=torch.int64, device="cuda")
    out_sc = torch.zeros((nql, K), dtype=torch.float64, device="cuda")
    out_cnt = torch.zeros(nql, dtype=torch.int32, device="cuda")
    out_msz = torch.zeros(nql, dtype=torch.int32, device="cuda")
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = (out_ids.data_ptr(), out_sc.data_ptr(), out_cnt.data_ptr(), out_msz.data_ptr())
    torch.cuda.synchronize()

    def sync():
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()

    info = None
    for i in range(args.warmup):
        info = rr.step(needs[i % len(needs)], qsets[i % len(qsets)], cfg_run, nql, K, shard_k, now_ms, out, d_bad.data_ptr())
    sync()
    t0 = time.perf_counter()
    cand = sent = recvd = scanned = 0
    for i in range(args.steps):
        info = rr.step(needs[i % len(needs)], qsets[i % len(qsets)], cfg_run, nql, K, shard_k, now_ms, out, d_bad.data_ptr())
        cand += int(out_cnt.sum().item())
        sent += info["postings_sent"]; recvd += info["postings_received"]; scanned += info["postings_scanned"]
    sync()
    elapsed = time.perf_counter() - t0
    tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    tc = torch.tensor([cand, int(d_bad.item()), sent, scanned], dtype=torch.int64, device="cuda")
    dist.all_reduce(tc, op=dist.ReduceOp.SUM)
    elapsed = float(tt.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out_ids.cpu().numpy(), out_sc.cpu().numpy(), out_cnt.cpu().numpy(), out_msz.cpu().numpy())
    # --full: the last batch against the unsharded index (rank 0's own queries)
    same = None
    if args.full and rank == 0:
        o, c, s = qsets[(args.steps - 1) % len(qsets)]
        qf = pkg.QueryBatch(index, o[:nql + 1], c[:o[nql]], s[:o[nql]], cfg, now_ms=now_ms)
        qf.run(); qf.finish()
        f_ids, f_sc, f_cnt, f_msz = qf.results()
        qf.close()
        ids, scores, counts, msz = out_ids.cpu().numpy(), out_sc.cpu().numpy(), out_cnt.cpu().numpy(), out_msz.cpu().numpy()
        same = bool(np.array_equal(f_cnt, counts) and np.array_equal(f_msz, msz) and np.array_equal(f_ids, ids) and
                    np.array_equal(f_sc.view(np.int64), scores.view(np.int64)))
    rr.close()
    if rank == 0:
        line = {
            "metric": "candidates/sec + recall@400, 100M-tweet SimClusters-ANN @1/2/4/8 GPU", "value": int(tc[0].item()) / elapsed,
            "unit": "candidates/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"batched simclusters-ann, {nq} concurrent user queries, {args.tweets} tweets x 144428 clusters, top-400, N=50 M=800 "
                                   f"{args.alg}, {world}xMI355X cluster-id-range shards: scanned prefixes exchanged by tweet hash over RCCL every batch, "
                                   f"temporary index, owners' proving merge",
                       "queries": nq, "tweets": args.tweets, "clusters": 144428, "k": 400, "sharding": "cluster-range", "shard_list_length": shard_k,
                       "queries_not_proven_by_cut_lists": int(tc[1].item()), "rotated_query_batches": len(qsets)},
            "queries_per_sec": nq * args.steps / elapsed, "postings_per_sec": int(tc[3].item()) / elapsed,
            "exchange_postings_per_step_all_gpus": int(tc[2].item()) / max(args.steps, 1),
            "exchange_bytes_per_gpu_per_step": int(tc[2].item()) * 16 / max(args.steps, 1) / world,
            "sharded_equals_unsharded": same, "fallback_units": info["fallback_units"] if info else 0,
            "roofline": None, "cpu_baseline": None, "corpus_build_s": t_corpus, "full": args.full,
        }
        os.write(json_fd, (json.dumps(line) + "\n").encode())
    dist.barrier()
    lib.sann_comm_destroy(comm)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="sann", choices=["sann", "dense", "hnsw"],
                    help="sann (default): the headline metric of BASELINE.json (configs[2]); dense / hnsw: the two legs of "
                         "configs[3], run through tools/dense_bench.py / tools/hnsw_bench.py on one GPU (their own JSON lines)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tweets", type=int, default=int(os.environ.get("SANN_BENCH_TWEETS", 100_000_000)))
    ap.add_argument("--corpus", default="device", choices=["device", "numpy"],
                    help="device: generated + indexed on the GPU (any size); numpy: host generator (<= a few M tweets)")
    ap.add_argument("--queries-per-gpu", type=int, default=1024)
    ap.add_argument("--alg", default="cosine", choices=["cosine", "logcosine", "dot"])
    ap.add_argument("--partitions", type=int, default=0, help="partitions per cluster list at N = 1 (0 = 32); divided by N when sharded")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target wall time of the CPU baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--check-queries", type=int, default=16, help="queries checked bit-for-bit against the oracle")
    ap.add_argument("--quality-queries", type=int, default=8,
                    help="queries whose result is compared with the exact full-cosine top-400 (device brute force over "
                         "every tweet's full embedding; N = 1 and --corpus device only; 0 = skip)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (the real multi-GPU path); gloo = host-staged exchange, only to "
                         "rehearse the N > 1 code path with several ranks sharing one GPU")
    ap.add_argument("--exercise-exchange", action="store_true",
                    help="N = 1 only: run the sharded path (process group, all-to-all, owner merge) with one shard")
    ap.add_argument("--sharding", default="tweet-hash", choices=["tweet-hash", "cluster-range"],
                    help="N > 1 (or --exercise-exchange): tweet-hash shards (the deployment: no data moves before the top-k) or the "
                         "cluster-id-range shards north_star names (every batch moves the scanned lists' top-M prefixes to the GPU "
                         "their tweets hash to: exact, and 17x the exchange bytes -- DESIGN.md section 4)")
    ap.add_argument("--quality-topical-tweets", type=int, default=1_000_000,
                    help="size of the topic-mixture corpus of the second quality field (recall_at_400_quality_topical); 0 = skip")
    ap.add_argument("--inflight", type=int, default=2, help="batches in flight: consecutive steps alternate between this many HIP streams")
    ap.add_argument("--rotate", type=int, default=8,
                    help="distinct prepared query batches the timed loop rotates through (each its own 1024*N synthetic users): 8 "
                         "batches scan ~1.9 GB of distinct postings, beyond L2 (32 MB) + Infinity Cache (256 MB), so no step finds "
                         "its postings cached from its own previous run; 1 = replay one batch (round 1-2 behaviour)")
    ap.add_argument("--serial-kernels", action="store_true",
                    help="batches in flight, but a batch's unit kernel waits for the previous batch's merge kernel (only the descriptor kernel and the host overlap)")
    ap.add_argument("--no-overlap", action="store_true", help="one batch at a time on one stream (and, sharded, exchange and owner merge on that stream too)")
    ap.add_argument("--shard-k", type=int, default=0, help="override the per-shard list length of sharded runs (0 = k/N + 6 sigma + 8)")
    ap.add_argument("--e2e-steps", type=int, default=-1,
                    help="steps of the end-to-end leg: fresh queries every step through sann_get_tweet_candidates, host buffers in "
                         "and out (N = 1 only; -1 = as many as --steps, 0 = skip)")
    ap.add_argument("--e2e-threads", type=int, default=4, help="concurrent callers of the end-to-end leg (the reference's callers are Finagle worker threads)")
    ap.add_argument("--e2e-query-sets", type=int, default=4, help="distinct query batches the end-to-end leg rotates through")
    ap.add_argument("--mb-threads", type=int, default=8, help="caller threads of the micro-batched leg (0 = skip)")
    ap.add_argument("--mb-window", type=int, default=128, help="single requests each caller thread keeps in flight (outstanding Futures)")
    ap.add_argument("--mb-requests", type=int, default=524288, help="single requests of the micro-batched leg, all threads together")
    ap.add_argument("--mb-batch", type=int, default=1024, help="max_batch of the micro-batching queue in that leg")
    ap.add_argument("--mb-wait-us", type=int, default=200, help="max_wait_us of the micro-batching queue in that leg")
    ap.add_argument("--mb-dispatchers", type=int, default=3)
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of the CPU baseline (0 = min(cpu_count, 16))")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything beside the headline: per-kernel timings "
                         "(roofline), the end-to-end and micro-batched legs, oracle parity, both recall fields, the CPU baseline "
                         "and, sharded, the comparison with the unsharded index (the options above tune these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (ids, scores, counts, map sizes) as DIR/<name>.npy, float64")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.workload != "sann" and args.dump_outputs:
        ap.error("--dump-outputs is for --workload sann")
    if args.workload != "sann":
        import subprocess
        tool = os.path.join(ROOT, "tools", "dense_bench.py" if args.workload == "dense" else "hnsw_bench.py")
        sys.exit(subprocess.run([sys.executable, tool, "--steps", str(max(1, min(args.steps, 5)))]).returncode)

    # batches in flight use a few HIP streams (two batch streams, the exchange stream, RCCL's own); the runtime
    # multiplexes streams onto 4 hardware queues by default, and two streams on one queue run in order
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with torch.distributed.run", file=sys.stderr)
        sys.exit(2)

    # --exercise-exchange: a 1-GPU run that still goes through process-group init, the all-to-all and the owner's
    # merge (one shard), so the RCCL plumbing of the N > 1 path can be checked on a 1-GPU box
    sharded = world > 1 or args.exercise_exchange
    dist = torch = None
    json_fd = None
    if sharded:
        # RCCL prints a version banner on STDOUT when the first communicator of the process comes up (through torch's
        # process group or through the library's own), and so does gloo ("[Gloo] Rank 0 is connected to ...").  This
        # program's stdout is ONE JSON line: file descriptor 1 is pointed at stderr for the rest of the run and the JSON
        # line goes to a private copy of the original.
        sys.stdout.flush()
        json_fd = os.dup(1)
        os.dup2(2, 1)
    if sharded:
        for key, val in (("RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29533")):
            os.environ.setdefault(key, val)
        import torch
        import torch.distributed as dist

        if args.backend == "gloo":
            local_rank = local_rank % max(torch.cuda.device_count(), 1)  # ranks may share a GPU in a rehearsal
            torch.cuda.set_device(local_rank)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        os.environ.setdefault("SANN_NO_TORCH", "1")  # torch-free: system HIP runtime, profiler-friendly

    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    pkg = ge.load_package()
    lib = pkg.load_library()
    SA = pkg.ScoringAlgorithm
    alg = {"cosine": SA.CosineSimilarity, "logcosine": SA.LogCosineSimilarity, "dot": SA.DotProduct}[args.alg]

    # ---- synthetic corpus + queries; identical on every rank ---------------------
    t0 = time.time()
    nq = args.queries_per_gpu * world
    nql = args.queries_per_gpu  # queries this rank owns (finalises); it still answers all nq on its shard
    range_mode = args.sharding == "cluster-range" and (world > 1 or args.exercise_exchange)
    p_full = args.partitions
    if world > 1:
        # a shard holds 1/world of every posting list: keep the (query, partition) units about the same size by
        # partitioning the shard world times less finely, down to 4 partitions (measured with tools/shard_cost.py on the
        # round-2 kernels, GPU-side step per 1024*N-query batch: N = 2: P = 32 / 16 / 8 -> 0.345 / 0.268 / 0.264 ms;
        # N = 4: P = 16 / 8 / 4 -> 0.374 / 0.290 / 0.270; N = 8: P = 8 / 4 -> 0.383 / 0.308; no unit falls back in any)
        p = max(4, (args.partitions or 32) // world)
        args.partitions = 1 << (p.bit_length() - 1)
    # query sets: set 0 is SURVEY 8(d)'s batch (seed 20260105); sets 1.. are further draws of the same user model
    n_rot = max(1, args.rotate)
    n_sets = max(n_rot, args.e2e_query_sets if not (world > 1 or args.exercise_exchange) else 1)
    offs, cids, scs = pkg.corpus.make_queries(nq)
    qsets = [(offs, cids, scs)]
    if n_sets > 1:
        o_all, c_all, s_all = pkg.corpus.make_queries(nq * (n_sets - 1), seed=pkg.corpus.QUERY_SEED + 1)
        for i in range(n_sets - 1):
            lo, hi = o_all[i * nq], o_all[(i + 1) * nq]
            qsets.append((o_all[i * nq:(i + 1) * nq + 1] - lo, c_all[lo:hi], s_all[lo:hi]))
    now_ms = pkg.corpus.NOW_MS
    if args.corpus == "device":
        # cluster-range ranks each generate the whole corpus (the generator has no range filter) and serve only their range
        index = pkg.ClusterTweetIndex.synthetic(args.tweets, pkg.corpus.N_CLUSTERS, seed=pkg.corpus.CORPUS_SEED,
                                                index_cap=2000, now_ms=now_ms, device=local_rank,
                                                n_partitions=p_full if range_mode else args.partitions, shard_id=0 if range_mode else rank,
                                                n_shards=1 if range_mode else world)
        co = None
    else:
        co = pkg.corpus.make_corpus(args.tweets)
        index = pkg.ClusterTweetIndex(co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores, device=local_rank,
                                      n_partitions=args.partitions, shard_id=rank, n_shards=world)
    t_corpus = time.time() - t0

    def host_lists(n_queries):
        """CSR posting lists (as the reference's store returns them) covering the first n queries."""
        if co is not None:
            return co.cluster_ids, co.list_offsets, co.tweet_ids, co.scores
        if world > 1:
            raise RuntimeError("host export of a sharded device index is not supported")
        return index.export_lists(cids[:offs[n_queries]])

    # cr-mixer default config with maxNumResults = 400
    cfg = pkg.SimClustersANNConfig(maxNumResults=400, minScore=0.0, maxTopTweetsPerCluster=800, maxScanClusters=50,
                                   maxTweetCandidateAgeHours=24, minTweetCandidateAgeHours=0, annAlgorithm=alg)
    # Sharded runs: a shard holds about K / world of a query's final top-K (tweets are hashed to shards), so it
    # delivers only its top shard_k = K/world + 6 sigma + 8 -- the per-shard merge, the exchange and the owner's merge
    # all shrink by K / shard_k -- and the owner PROVES the merged top-K exact from the cut lists
    # (sann_merge_shards_cut); a batch that cannot be proven is redone with shard_k = K.
    K = cfg.maxNumResults
    shard_k = K
    if world > 1:
        shard_k = pkg.sharding.shard_list_length(K, world)
    if args.shard_k > 0 and sharded:
        shard_k = min(K, args.shard_k)
    # streams are made once (a repeated measurement must not add streams: more streams than hardware queues share
    # queues, and two streams on one queue run in order)
    depth = 1 if args.no_overlap else max(1, args.inflight)
    side_stream = None
    if sharded:
        t_streams = [torch.cuda.current_stream()] if depth == 1 else [torch.cuda.Stream() for _ in range(depth)]
        streams = [t.cuda_stream for t in t_streams]
        side_stream = t_streams[0] if args.no_overlap else torch.cuda.Stream()
    elif depth == 1:
        streams = [0]
    else:
        hip = ctypes.CDLL("libamdhip64.so")
        streams = []
        for _ in range(depth):
            h_stream = ctypes.c_void_p()
            assert hip.hipStreamCreateWithFlags(ctypes.byref(h_stream), 1) == 0  # hipStreamNonBlocking
            streams.append(h_stream.value)
    comm = None
    if sharded and args.backend != "gloo":
        # the library's RCCL communicator; torch.distributed only carries the 128-byte unique id (and the barriers)
        uid = [None]
        if rank == 0:
            buf = ctypes.create_string_buffer(128)
            assert lib.sann_comm_unique_id(buf) == 0, lib.sann_last_error()
            uid[0] = buf.raw
        dist.broadcast_object_list(uid, src=0)
        comm = ctypes.c_void_p()
        rc = lib.sann_comm_create(local_rank, rank, world, uid[0], ctypes.byref(comm))
        assert rc == 0, lib.sann_last_error()
    if args.sharding == "cluster-range" and sharded:
        return run_cluster_range(args, pkg, lib, index, comm, dist, torch, rank, world, local_rank, nq, nql, qsets[:n_rot], cfg, K, shard_k,
                                 now_ms, json_fd, t_corpus)
    inexact_seen = 0
    while True:
        cfg_run = cfg if shard_k == K else dataclasses.replace(cfg, maxNumResults=shard_k)
        # Batches in flight: consecutive steps alternate between `depth` QueryBatch objects (own workspaces and
        # outputs, same queries) on their own HIP streams, so the GPU always has the next batch queued: batch i+1's
        # descriptor / unit kernels run beside batch i's merge kernel (LDS-bound, one round of workgroups), and the
        # host's per-batch stream wait + status check (sann_batch_finish) is off the GPU's critical path.  Every batch
        # is complete (finished, checked, and when sharded exchanged and merged) before the timed region ends.
        # `depth` streams, `n_rot` prepared batches (own workspaces and outputs, DISTINCT queries): step s runs batch
        # s % n_rot on stream s % depth
        n_obj = max(depth, n_rot)
        qbs = [pkg.QueryBatch(index, *qsets[j % n_rot], cfg_run, now_ms=now_ms) for j in range(n_obj)]
        stride = qbs[0].stride
        launched = []  # (batch, stream slot) enqueued but not yet finished, oldest first
        n_steps_done = [0]
        alone = [False]  # True: one batch at a time, nothing overlapped (the per-kernel timings after the timed region)

        # ---- multi-GPU plumbing: per-shard answers -> all-to-all by query owner -> exact merge ----------
        # Rank r owns queries [r*nql, (r+1)*nql).  Every rank answers all nq queries on its tweet-hash shard;
        # the merge kernel writes query q's results straight into the message of its owner, and ONE all-to-all
        # (RCCL over xGMI: (world-1)/world of nq*shard_k*16 B leaves each GPU, the same amount arrives) delivers
        # them; the owner merges world per-shard lists.  Exchange and owner merge run on a side stream.
        if sharded:
            # one packed message per owner: [ids nql*stride | score bits nql*stride | counts nql | map sizes nql]
            chunk, _offsets = pkg.sharding.owner_message_layout(nql, stride)  # bytes, a multiple of 8
            arr = nql * stride * 8
            sends = [torch.zeros(world * chunk, dtype=torch.uint8, device="cuda") for _ in range(n_obj)]
            recv = torch.zeros_like(sends[0])  # [world shards][chunk]: this rank's queries, one chunk per shard
            rp = recv.data_ptr()
            sent = [None] * n_obj  # event: the exchange that read sends[batch] has finished
            ready = [torch.cuda.Event() for _ in sends]  # event: the batch in sends[slot] is final
            for j, qb in enumerate(qbs):
                sp = sends[j].data_ptr()
                qb.bind_outputs_chunked(sp, sp + arr, sp + 2 * arr, sp + 2 * arr + 4 * nql, nql, chunk)
            out_ids = torch.zeros((nql, K), dtype=torch.int64, device="cuda")
            out_sc = torch.zeros((nql, K), dtype=torch.float64, device="cuda")
            out_cnt = torch.zeros(nql, dtype=torch.int32, device="cuda")
            out_msz = torch.zeros(nql, dtype=torch.int32, device="cuda")
            d_ks = [qb.device_k() + rank * nql * 4 for qb in qbs]
            d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")  # queries whose cut per-shard lists could not prove the merge exact
            torch.cuda.synchronize()  # the buffers were zero-filled on the default stream; they are used on others

        def exchange(send, recv, stream_ptr):
            if args.backend == "gloo":  # rehearsal: gloo has no all-to-all; gather on the host and slice
                h = send.cpu()
                parts = [torch.zeros_like(h) for _ in range(world)]
                dist.all_gather(parts, h)
                c = h.numel() // world
                recv.copy_(torch.cat([p[rank * c:(rank + 1) * c] for p in parts]))
            else:  # the library's own RCCL exchange (csrc/sann_comm.hip): what a non-Python worker calls too
                rc = lib.sann_exchange_to_owners(comm, ctypes.c_void_p(stream_ptr), ctypes.c_void_p(send.data_ptr()),
                                                 ctypes.c_void_p(recv.data_ptr()), chunk)
                assert rc == 0, lib.sann_last_error()

        def post(j, slot):
            """Exchange + owner merge of a finished batch, on the side stream."""
            ready[j].record(t_streams[slot])
            with torch.cuda.stream(side_stream):
                side_stream.wait_event(ready[j])
                exchange(sends[j], recv, side_stream.cuda_stream)
                sent[j] = torch.cuda.Event()
                sent[j].record(side_stream)
                side = ctypes.c_void_p(side_stream.cuda_stream)
                if shard_k < K:
                    rc = lib.sann_merge_shards_cut(local_rank, side, world, nql, stride, chunk, shard_k, K, K,
                                                   rp, rp + arr, rp + 2 * arr, rp + 2 * arr + 4 * nql,
                                                   out_ids.data_ptr(), out_sc.data_ptr(), out_cnt.data_ptr(), out_msz.data_ptr(),
                                                   d_bad.data_ptr())
                else:
                    rc = lib.sann_merge_shards(local_rank, side, world, nql, stride, chunk, rp, rp + arr,
                                               rp + 2 * arr, rp + 2 * arr + 4 * nql,
                                               d_ks[j], out_ids.data_ptr(), out_sc.data_ptr(), out_cnt.data_ptr(), out_msz.data_ptr())
                assert rc == 0, lib.sann_last_error()

        def retire(j, slot):
            # waits for the batch's stream and re-runs whatever the fast path flagged, before anything is sent
            qbs[j].finish(streams[slot])
            if sharded:
                post(j, slot)

        prev = [None]   # the batch of the previous step (its unit kernel is what this step's unit kernel waits for)
        runs = [0] * n_obj  # timed steps each batch object served

        def step(force_j=None):
            s_no = n_steps_done[0]
            slot, j = s_no % depth, (s_no % n_obj if force_j is None else force_j)
            n_steps_done[0] += 1
            runs[j] += 1
            if sharded and sent[j] is not None:
                t_streams[slot].wait_event(sent[j])  # the message buffer is free again
            # asynchronous: descriptor, unit and merge kernels of this batch; the unit kernel waits on the GPU for the
            # previous batch's unit kernel (the dominant kernels run one at a time, everything else overlaps)
            if depth > 1 and not alone[0] and prev[0] is not None:
                qbs[j].run_after(streams[slot], qbs[prev[0]], after_merge=args.serial_kernels)
            elif depth > 1 and not alone[0]:
                qbs[j].run_after(streams[slot], None, after_merge=args.serial_kernels)
            else:
                qbs[j].run(streams[slot])
            prev[0] = j
            launched.append((j, slot))
            # keep depth-1 batches queued behind the one the host now waits for (none when timing kernels alone)
            while len(launched) > (0 if alone[0] else depth - 1):
                retire(*launched.pop(0))

        def sync():
            while launched:
                retire(*launched.pop(0))
            if sharded:
                torch.cuda.synchronize()
                dist.barrier()
                torch.cuda.synchronize()
            else:
                assert lib.sann_device_synchronize(local_rank) == 0

        def check_sharded_against_unsharded():
            """Sharded runs, after the timed region: rank 0 also builds the whole corpus on its GPU and checks the merged
            answer of the queries it owns, bit for bit (the other ranks wait at the final barrier)."""
            full = pkg.ClusterTweetIndex.synthetic(args.tweets, pkg.corpus.N_CLUSTERS, seed=pkg.corpus.CORPUS_SEED,
                                                   index_cap=2000, now_ms=now_ms, device=local_rank, n_partitions=args.partitions)
            qf = pkg.QueryBatch(full, offs[:nql + 1], cids[:offs[nql]], scs[:offs[nql]], cfg, now_ms=now_ms)
            qf.run(); qf.finish()
            f_ids, f_sc, f_cnt, f_msz = qf.results()
            qf.close(); full.close()
            return bool(np.array_equal(f_cnt, counts) and np.array_equal(f_msz, msz) and np.array_equal(f_ids, ids)
                        and np.array_equal(f_sc.view(np.int64), scores.view(np.int64)))

        for _ in range(args.warmup):
            step()
        # the timed region carries HIP events around the dominant kernel only (two per step; each event costs the
        # stream ~5 us), with or without --full, so that ms_per_step is the same measurement either way; --full times
        # the descriptor and merge kernels over a few extra steps afterwards
        sync()
        for qb in qbs:
            qb.set_profiling(1)
        for j in range(n_obj):
            runs[j] = 0
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        sync()
        elapsed = time.perf_counter() - t0
        runs_timed = list(runs)
        if args.dump_outputs and rank == 0:
            # the last timed step's answer (sharded: the owner's merged answer of this rank's queries)
            last = ((out_ids.cpu().numpy(), out_sc.cpu().numpy(), out_cnt.cpu().numpy(), out_msz.cpu().numpy()) if sharded
                    else qbs[prev[0]].results())
            dump_outputs(args.dump_outputs, *last)
        unit_ms = sum(qb.kernel_times()[0] for qb in qbs)
        n_timed = sum(qb.kernel_times()[2] for qb in qbs)
        if args.full:
            for qb in qbs:
                qb.set_profiling(2)
            alone[0] = True  # a few more steps, one batch at a time: each kernel's duration with the GPU to itself
            n_aux = max(3, min(10, args.steps))
            for _ in range(n_aux):
                step()
            sync()
            alone[0] = False
            unit_alone_ms = sum(qb.kernel_times()[0] for qb in qbs) / n_aux
            merge_ms = sum(qb.kernel_times()[1] for qb in qbs)
            desc_ms = sum(qb.desc_time() for qb in qbs)
            merge_ms, desc_ms = merge_ms * n_timed / n_aux, desc_ms * n_timed / n_aux  # reported as per-launch averages below
        for qb in qbs:
            qb.set_profiling(False)
        # ---- results: candidates every prepared batch returns (the rotated batches differ), and batch 0's answer (query
        # set 0 = SURVEY 8(d)'s seed; this rank's own queries when sharded) for the checks below ----------------------
        cand_of = [0] * n_obj
        if sharded:
            # the owners' merged outputs are one buffer: one more pass, a batch at a time, batch 0 last
            alone[0] = True
            for j in reversed(range(n_obj)):
                step(force_j=j)
                sync()
                cand_of[j] = int(out_cnt.sum().item())
            alone[0] = False
            ids, scores, counts, msz = out_ids.cpu().numpy(), out_sc.cpu().numpy(), out_cnt.cpu().numpy(), out_msz.cpu().numpy()
        else:
            for j in reversed(range(n_obj)):
                ids, scores, counts, msz = qbs[j].results()
                cand_of[j] = int(counts.sum())
        n_fallback_units = sum(int(qb.stats().n_fallback_units) for qb in qbs)
        n_runs_timed = max(sum(runs_timed), 1)
        candidates_timed = sum(r * c for r, c in zip(runs_timed, cand_of))  # over the timed steps, this rank's queries
        # per-launch averages over the timed steps (sum_q P_q*16 + n*12, + k_out*16 added below)
        postings_per_step = sum(r * int(qb.stats().postings_scanned) for r, qb in zip(runs_timed, qbs)) / n_runs_timed
        alg_bytes = int(sum(r * (int(qb.stats().algorithmic_bytes) + c * 16) for r, qb, c in zip(runs_timed, qbs, cand_of)) / n_runs_timed)
        if sharded:
            dev = "cpu" if args.backend == "gloo" else "cuda"
            tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = float(tt.item())
            tc = torch.tensor([candidates_timed, int(d_bad.item())], dtype=torch.int64, device=dev)
            dist.all_reduce(tc, op=dist.ReduceOp.SUM)
            candidates_timed = int(tc[0].item())  # whole job: every rank's queries
            if int(tc[1].item()) > 0 and shard_k < K:
                # some query's merged top-k could not be proven exact from the cut lists: the whole measurement
                # is repeated with full-length per-shard lists (expected never; the proof is checked every batch)
                inexact_seen += int(tc[1].item())
                shard_k = K
                for qb in qbs:
                    qb.close()
                continue
        break
    value = candidates_timed / elapsed

    # ---- end-to-end leg: the boundary call itself, fresh queries every step ---------------------------------------
    # sann_get_tweet_candidates = host arrays in -> packed H2D -> device-side query preparation -> descriptor / unit /
    # merge kernels -> D2H of the results into (pinned) host arrays, from --e2e-threads concurrent callers, each with
    # its own pooled batch object and stream.  Reported beside `value`, never instead of it: PCIe-inclusive.
    e2e = None
    n_e2e = args.steps if args.e2e_steps < 0 else args.e2e_steps
    if args.full and not sharded and n_e2e > 0:
        import threading

        sa = pkg.simclusters_ann
        n_thr = max(1, args.e2e_threads)
        outs = [(sa.pinned_array((nq, K), np.int64), sa.pinned_array((nq, K), np.float64), sa.pinned_array((nq,), np.int32),
                 sa.pinned_array((nq,), np.int32)) for _ in range(n_thr)]
        cand_total = [0] * n_thr
        first_answer = [None]

        def caller(t, steps, record):
            for i in range(steps):
                qs = qsets[(t + i * n_thr) % n_sets]
                ids_e, sc_e, cnt_e, msz_e = sa.get_tweet_candidates(index, *qs, cfg, now_ms=now_ms, out=outs[t])
                if record:
                    cand_total[t] += int(cnt_e.sum())
                    if t == 0 and i == 0:
                        first_answer[0] = (ids_e.copy(), sc_e.copy(), cnt_e.copy(), msz_e.copy())

        def run_callers(total_steps, record):
            per = [total_steps // n_thr + (1 if t < total_steps % n_thr else 0) for t in range(n_thr)]
            ths = [threading.Thread(target=caller, args=(t, per[t], record)) for t in range(n_thr)]
            for th in ths:
                th.start()
            for th in ths:
                th.join()

        run_callers(max(args.warmup, n_thr), False)
        assert lib.sann_device_synchronize(local_rank) == 0
        t0 = time.perf_counter()
        run_callers(n_e2e, True)
        assert lib.sann_device_synchronize(local_rank) == 0
        e2e_elapsed = time.perf_counter() - t0
        py_ms_per_step = e2e_elapsed / n_e2e * 1e3
        # The same calls from NATIVE caller threads (tools/micro/batcher_load.c: e2e_load_run).  The Python callers above hold the
        # interpreter lock while they marshal a call's arguments (~0.1 ms, half a GPU step), so what they time is the harness;
        # the native callers time the library.  Same entry point, same query sets, same pinned response buffers.
        native = None
        load_so_e = os.path.join(ROOT, "tools", "micro", "libbatcher_load.so")
        if os.path.exists(load_so_e):
            ld = ctypes.CDLL(load_so_e)
            PP = ctypes.c_void_p * n_sets
            keep = [(np.ascontiguousarray(q[0], np.int64), np.ascontiguousarray(q[1], np.int32), np.ascontiguousarray(q[2], np.float64)) for q in qsets[:n_sets]]
            a_o, a_c, a_s = PP(*[k_[0].ctypes.data for k_ in keep]), PP(*[k_[1].ctypes.data for k_ in keep]), PP(*[k_[2].ctypes.data for k_ in keep])
            ld.e2e_load_run.restype = ctypes.c_int
            ld.e2e_load_run.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]
            cfg_e = cfg.to_c()
            r3 = (ctypes.c_double * 3)()
            n_nat = max(10 * n_e2e, 400)  # (0.1 s of calls: the pipeline's ramp-up -- the first few calls -- is not what is measured)
            for n_calls in (2 * n_thr, n_nat):
                rc = ld.e2e_load_run(index.handle, n_thr, n_calls, nq, n_sets, a_o, a_c, a_s, ctypes.byref(cfg_e), now_ms, r3)
                assert rc == 0, lib.sann_last_error()
            native = (r3[0] / r3[1] * 1e3, r3[2] / r3[0], int(r3[1]))
            if os.environ.get("SANN_TRACE_CALLS") == "1":
                us4, n_tr = (ctypes.c_double * 4)(), ctypes.c_int64()
                lib.sann_debug_call_trace(us4, ctypes.byref(n_tr))
                print(f"e2e trace: {n_tr.value} calls; per call submit {us4[0] / max(n_tr.value, 1):.0f} us, enqueue copies {us4[1] / max(n_tr.value, 1):.0f} us, "
                      f"wait kernels {us4[2] / max(n_tr.value, 1):.0f} us, wait copies {us4[3] / max(n_tr.value, 1):.0f} us", file=sys.stderr)
            e2e_elapsed, n_e2e_timed = r3[0], int(r3[1])
            cand_total = [int(r3[2])]
        else:
            n_e2e_timed = n_e2e
        # thread 0's first call answered query set 0 = the replayed batch: must be the same answer, bit for bit
        fa = first_answer[0]
        same = bool(np.array_equal(fa[2], counts) and np.array_equal(fa[3], msz) and
                    all(np.array_equal(fa[0][q, :counts[q]], ids[q, :counts[q]]) and
                        np.array_equal(fa[1][q, :counts[q]].view(np.int64), scores[q, :counts[q]].view(np.int64)) for q in range(nq)))
        # one caller alone: the latency of a single call
        t1 = time.perf_counter()
        n_lat = max(3, min(10, n_e2e))
        for i in range(n_lat):
            sa.get_tweet_candidates(index, *qsets[i % n_sets], cfg, now_ms=now_ms, out=outs[0])
        lat_ms = (time.perf_counter() - t1) / n_lat * 1e3
        e2e = {"value": sum(cand_total) / e2e_elapsed, "unit": "candidates/sec", "ms_per_step": e2e_elapsed / n_e2e_timed * 1e3,
               "steps": n_e2e_timed, "callers": n_thr, "caller_threads": "native (pthreads)" if native else "python",
               "python_callers_ms_per_step": py_ms_per_step, "fresh_query_sets": n_sets, "single_call_latency_ms": lat_ms,
               "equals_replayed_batch": same, "ratio_to_replay_step": (e2e_elapsed / n_e2e_timed) / (elapsed / args.steps),
               "what": "sann_get_tweet_candidates per step: pageable host query arrays in, packed H2D, device-side query "
                       "preparation, descriptor + unit + merge kernels, D2H of ids/scores/counts into pinned host arrays; "
                       "pooled batch objects, no allocation in steady state"}

    # ---- micro-batched leg: SINGLE requests from many native caller threads through the micro-batching queue ----------
    # (the reference's calling pattern: one getTweetCandidates per Finagle worker thread at a time,
    # SimClustersANNCandidateSource.scala:77-94).  tools/micro/batcher_load.c drives sann_batcher_get_tweet_candidates from
    # pthreads; Python only sets it up.  Reported beside `value`, never instead of it.
    mb_leg = None
    load_so = os.path.join(ROOT, "tools", "micro", "libbatcher_load.so")
    if args.full and not sharded and n_e2e > 0 and args.mb_threads > 0 and os.path.exists(load_so):
        load = ctypes.CDLL(load_so)
        load.batcher_load_run.restype = ctypes.c_int
        load.batcher_load_run.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)]
        mb = pkg.MicroBatcher(index, max_batch=args.mb_batch, max_wait_us=args.mb_wait_us, n_dispatchers=args.mb_dispatchers)
        cfg_c = cfg.to_c()
        o_q, c_q, s_q = (np.ascontiguousarray(qsets[0][0], np.int64), np.ascontiguousarray(qsets[0][1], np.int32),
                         np.ascontiguousarray(qsets[0][2], np.float64))
        res = (ctypes.c_double * 6)()
        per = max(2 * args.mb_window, args.mb_requests // args.mb_threads)
        for n_req in (2 * args.mb_window, per):  # a short warm-up run, then the measured one
            rc = load.batcher_load_run(mb._h, args.mb_threads, args.mb_window, n_req, nq, o_q.ctypes.data, c_q.ctypes.data, s_q.ctypes.data,
                                       ctypes.byref(cfg_c), now_ms, res)
            assert rc == 0, lib.sann_last_error()
        st_mb = mb.stats()
        mb.close()
        mb_leg = {"value": res[2] / res[0], "unit": "candidates/sec", "requests_per_sec": res[1] / res[0], "requests": int(res[1]),
                  "caller_threads": args.mb_threads, "requests_in_flight_per_caller": args.mb_window, "latency_us_p50": res[3], "latency_us_p99": res[4], "latency_us_max": res[5],
                  "max_batch": args.mb_batch, "max_wait_us": args.mb_wait_us, "dispatchers": args.mb_dispatchers,
                  "mean_batch": st_mb.n_requests / max(st_mb.n_batches, 1), "batches_closed_full": int(st_mb.n_closed_full),
                  "batches_closed_by_deadline": int(st_mb.n_closed_by_deadline),
                  "what": "single getTweetCandidates requests through sann_submit / sann_wait from native caller threads that each keep a "
                          "window of requests in flight (tools/micro/batcher_load.c), folded into batches by the library's micro-batching "
                          "queue; every request pays its copy into the open batch, the batch's whole boundary call and the copy of its rows; "
                          "latency = submit -> collected"}

    if rank != 0:
        if sharded:
            dist.barrier()
            if comm is not None:
                lib.sann_comm_destroy(comm)
            dist.destroy_process_group()
        return

    # ---- --full: parity spot check against the oracle (outside the timed region) ----------------
    oracle = ge.load_oracle() if args.full else None
    n_check = min(args.check_queries, nql) if args.full and (co is not None or world == 1) else 0
    exact = 0
    if n_check:
        L = host_lists(n_check)
        for q in range(n_check):
            o_ids, o_sc, o_msz = oracle.sann_query(cids[offs[q]:offs[q + 1]], scs[offs[q]:offs[q + 1]], None, cfg, now_ms, *L)
            ok = (counts[q] == len(o_ids) and msz[q] == o_msz and np.array_equal(ids[q, :counts[q]], o_ids)
                  and np.array_equal(scores[q, :counts[q]].view(np.int64), o_sc.view(np.int64)))
            exact += int(ok)
    recall_parity = exact / n_check if n_check else None

    # ---- quality recall@400: approximate top-400 vs the exact full-embedding cosine top-400 --
    recall_quality = None
    if args.full and world == 1 and co is None and args.quality_queries > 0 and args.alg == "cosine":
        nqq = min(args.quality_queries, nq)
        e_ids, _e_cos, e_cnt = index.exact_cosine_topk(offs[:nqq + 1], cids[:offs[nqq]], scs[:offs[nqq]], 400)
        hit = tot = 0
        for q in range(nqq):
            found = set(ids[q, :counts[q]].tolist())
            truth = e_ids[q, :e_cnt[q]].tolist()[:max(len(found), 1)]  # loadtest definition when shorter than k
            hit += len(found.intersection(truth))
            tot += min(len(found), len(truth)) if found else len(truth)
        recall_quality = hit / max(tot, 1)

    # ---- the same quality measure where the data has the structure the algorithm relies on: a topic-mixture corpus (tweets and
    #      users draw 90 % of their clusters from their topic's 64), host-generated at --quality-topical-tweets, the operator on
    #      the GPU vs the exact full cosine by scipy over every tweet's full embedding (tools/quality_topics.py) -----------------
    recall_topical = None
    if args.full and world == 1 and co is None and args.quality_topical_tweets > 0 and args.alg == "cosine":
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
        import quality_topics
        r = quality_topics.run(pkg, args.quality_topical_tweets, 32, 2000, 400, alg)
        recall_topical = {"value": r["recall_at_k_quality"], "min": r["min"], "max": r["max"], "tweets": r["tweets"], "queries": r["queries"],
                          "topics": r["n_topics"], "corpus": "corpus.make_corpus(n_topics=2000): 90 % of a tweet's / user's clusters from its topic's 64"}

    # ---- CPU baseline: the C restatement of the Scala path on the host cores, bounded sample ---
    cpu = None
    if args.full and not args.no_cpu_baseline and (co is not None or world == 1):
        # a 1-GPU box's CPU share is 16 cores even when 256 logical CPUs are visible
        cores = args.cpu_threads or min(os.cpu_count() or 1, 16)
        n_s = min(nq, 256)
        L = host_lists(n_s)
        o_i = np.zeros((n_s, 1000), np.int64)
        o_s = np.zeros((n_s, 1000), np.float64)
        o_c = np.zeros(n_s, np.int32)
        legs = {}
        for variant, name in ((0, "original"), (1, "optimized")):
            sec, reps, cands = 0.0, 0, 0
            while sec < args.cpu_seconds / 2 and reps < 10000:
                sec += oracle.baseline_run(variant, cores, offs[:n_s + 1], cids, scs, cfg, now_ms, *L, o_i, o_s, o_c)
                cands += int(o_c.sum())
                reps += 1
            legs[name] = (cands / sec, sec, reps)
        cpu = {"value": legs["original"][0], "unit": "candidates/sec", "cores": cores, "kind": "port",
               "optimized_value": legs["optimized"][0],
               "sample": f"the first {n_s} of the {nq} queries; 'original' (ApproximateCosineSimilarity: two hash maps, four probes per "
                         f"posting, full sort) x {legs['original'][2]} repetitions in {legs['original'][1]:.1f} s = `value`; 'optimized' "
                         f"(OptimizedApproximateCosineSimilarity: one map, two probes, full sort) x {legs['optimized'][2]} repetitions in "
                         f"{legs['optimized'][1]:.1f} s = `optimized_value`; {cores} threads; C restatement of the Scala CPU path, "
                         f"not the JVM (no boxing, allocation or GC modelled)"}

    # ---- --full: roofline of the dominant kernel (unit kernel: gather + accumulate + select) ---
    # algorithmic bytes per launch: sum_q P_q*16 + n*12 + k_out*16
    distinct_clusters = int(len(np.unique(np.concatenate([q[1] for q in qsets[:n_rot]]))))
    roof = None
    if args.full:
        unit_avg_ms = unit_ms / max(n_timed, 1)
        achieved = alg_bytes / (unit_avg_ms * 1e-3) / 1e9 if unit_avg_ms > 0 else 0.0
        roof = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic_bytes(args, nq, world), "kernel": "sann::unit_fast_kernel (gather+accumulate+select)",
                "kernel_avg_ms": unit_avg_ms, "desc_kernel_avg_ms": desc_ms / max(n_timed, 1),
                "merge_kernel_avg_ms": merge_ms / max(n_timed, 1), "algorithmic_bytes_per_launch": alg_bytes,
                # the timed region keeps batches in flight, so its unit kernel shares the GPU with the previous batch's
                # merge kernel and the next batch's descriptor kernel; *_alone = the same launch with the GPU to itself
                # (steps after the timed region, one batch at a time), as are the desc / merge figures above
                "frac_against": ("HBM3E 8 TB/s: the timed loop rotates %d distinct prepared batches (%d distinct scanned clusters, up to "
                                 "%.2f GB of distinct postings between two runs of the same batch), beyond L2 32 MB + Infinity Cache "
                                 "256 MB; the corpus's hottest clusters (Zipf head, shared by all batches) still hit in cache, as they "
                                 "would in service" % (n_rot, distinct_clusters, distinct_clusters * 800 * 16 / 1e9)) if n_rot >= 8 else
                                "HBM3E 8 TB/s, but the loop replays %d batch(es): their postings can stay in the 256 MB Infinity Cache" % n_rot,
                "kernel_avg_ms_alone": unit_alone_ms,
                "frac_alone": (alg_bytes / (unit_alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if unit_alone_ms > 0 else 0.0}

    line = {
        "metric": "candidates/sec + recall@400, 100M-tweet SimClusters-ANN @1/2/4/8 GPU",
        "value": value,
        "unit": "candidates/sec",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"batched simclusters-ann, {nq} concurrent user queries, {args.tweets} tweets x 144428 clusters, "
                               f"top-400, N=50 M=800 {args.alg}, {'1xMI355X' if world == 1 else f'{world}xMI355X tweet-hash shards + RCCL all-to-all merge'}",
                   "queries": nq, "tweets": args.tweets, "clusters": 144428, "k": 400, "max_scan_clusters": 50,
                   "max_top_tweets_per_cluster": 800, "algorithm": args.alg, "index_cap": 2000,
                   "partitions": index.info().n_partitions, "sharding": "none" if world == 1 else "tweet-hash",
                   "shard_list_length": shard_k, "queries_not_proven_by_cut_lists": inexact_seen,
                   "batches_in_flight": depth, "rotated_query_batches": n_rot,
                   "distinct_scanned_clusters_in_rotation": distinct_clusters,
                   "distinct_posting_bytes_in_rotation_upper": distinct_clusters * 800 * 16,
                   "corpus": args.corpus, "index_postings": int(index.info().n_postings_total)},
        "queries_per_sec": nq * args.steps / elapsed,
        "postings_per_sec": postings_per_step * args.steps / elapsed,
        "recall_at_400_parity": recall_parity,
        "recall_at_400_quality": recall_quality,
        "recall_at_400_quality_topical": recall_topical,
        "quality_checked_queries": (min(args.quality_queries, nq) if recall_quality is not None else 0),
        "parity_checked_queries": n_check,
        "fallback_units": n_fallback_units,
        "sharded_equals_unsharded": check_sharded_against_unsharded() if world > 1 and args.full else None,
        "roofline": roof,
        "end_to_end": e2e,
        "micro_batched": mb_leg,
        "cpu_baseline": cpu,
        "corpus_build_s": t_corpus,
        "full": args.full,
    }
    if json_fd is not None:
        os.write(json_fd, (json.dumps(line) + "\n").encode())
    else:
        print(json.dumps(line), flush=True)
    if sharded:
        dist.barrier()
        if comm is not None:
            lib.sann_comm_destroy(comm)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
