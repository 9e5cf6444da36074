/*
 * hnsw_update_ref.c -- CPU restatement of hnsw_index_update (include/hnsw_ann.h).  TEST INFRASTRUCTURE ONLY.
 *
 * Two restatements over the helpers of oracle/hnsw_oracle.c (queues, item distances, heuristic, graph rows), included unchanged:
 *   ref_hnsw_update(..., batch >= 1)   the device's rounds: per round 1 rows, 2 relink proposals against the graph as the round
 *                                      found it (the latest item in request order wins per (layer, v)), 3 the wiring walks with
 *                                      the items' own lists committed after all of them, 4 the builder's phase B with additions
 *                                      the list already holds dropped
 *   ref_hnsw_update(..., batch = 0)    HnswIndex.reInsert called once per row in request order, written straight from
 *                                      HnswIndex.java:226-329 (relink, then wireConnectionForAllLayers(..., isUpdate = true))
 *                                      and :384-440 / :571-623 with isUpdate = true
 * Both share the documented choices of this library: setCand in insertion order (the reference's HashSet order is unspecified),
 * a layer whose wiring heuristic keeps nobody keeps its old list and continues from u (the reference throws at :439), and the
 * walk's candidate-queue bound ccap of the device builder.  Paths are relative to ann/src/main/java/com/twitter/ann/hnsw/.
 */
#include "../oracle/hnsw_oracle.c"

#include <stdio.h>

typedef struct {
  int64_t n_relinks, n_superseded, n_present, n_kept;
} ustats;

static int imin(int a, int b) { return a < b ? a : b; }

/* :244-250: the highest layer <= maxLevel holding HnswNode(layer, u); -1 without HnswNode(0, u) (:239-240 checkState) */
static int top_of(const hbuild *g, int64_t u) {
  if (g->cnt[0][u] < 0) return -1;
  int top = 0;
  for (int l = 1; l <= g->max_level && l < g->n_levels; l++)
    if (g->cnt[l][u] >= 0) top = l;
  return top;
}

/* :256-277: setCand = u, then each e of N_l(u) followed by N_l(e), first occurrence kept */
static int set_cand(const hbuild *g, int level, int64_t u, int64_t *sc, uint8_t *mark) {
  int s = 0;
  sc[s++] = u;
  mark[u] = 1;
  const int64_t *l1;
  const int c1 = list_of(g, level, u, &l1);
  for (int i = 0; i < c1; i++) {
    const int64_t e = l1[i];
    if (!mark[e]) { mark[e] = 1; sc[s++] = e; }
    const int64_t *l2;
    const int c2 = list_of(g, level, e, &l2);
    for (int k = 0; k < c2; k++)
      if (!mark[l2[k]]) { mark[l2[k]] = 1; sc[s++] = l2[k]; }
  }
  for (int i = 0; i < s; i++) mark[sc[i]] = 0;
  return s;
}

/* :281-314: the new list of v from setCand \ {v} */
static int propose(const hbuild *g, int level, int64_t v, const int64_t *sc, int s, int64_t *out) {
  jpq q;
  jpq_init(&q, 0);
  const int keep = imin(g->efc, s - 1);
  for (int i = 0; i < s; i++) {
    if (sc[i] == v) continue;
    qitem it = {item_distance(g, v, sc[i]), sc[i]};
    if (q.n < keep) jpq_offer(&q, it);
    else if (it.d < q.a[0].d) { jpq_poll(&q); jpq_offer(&q, it); }
  }
  const int nk = select_by_heuristic(g, &q, v, level == 0 ? g->max_m0 : g->max_m, out);
  free(q.a);
  return nk;
}

/* :571-623 with isUpdate = true, and the device builder's candidate-queue bound */
static void search_layer_update(const hbuild *g, int64_t item, int64_t entry, int ef, int level, uint8_t *visited, jpq *wq, int ccap) {
  jpq cq;
  jpq_init(&cq, 1);
  jpq_init(wq, 0);
  qitem first = {item_distance(g, item, entry), entry};
  jpq_offer(&cq, first);
  jpq_offer(wq, first);
  memset(visited, 0, (size_t)g->n);
  visited[entry] = 1;
  float lower = wq->a[0].d;
  while (cq.n > 0) {
    qitem cand = cq.a[0];
    if (cand.d > lower) break;
    jpq_poll(&cq);
    const int64_t *list;
    int ln = list_of(g, level, cand.item, &list);
    for (int j = 0; j < ln; j++) {
      int64_t nn = list[j];
      if (visited[nn]) continue;
      visited[nn] = 1;
      float dist = item_distance(g, item, nn);
      if (wq->n < ef || dist < wq->a[0].d) {
        qitem it = {dist, nn};
        if (cq.n >= ccap) {
          int had = cq.n;
          qitem *old = malloc(sizeof(qitem) * (size_t)had);
          memcpy(old, cq.a, sizeof(qitem) * (size_t)had);
          cq.n = 0;
          for (int s = 0; s < had; s++) if (!(old[s].d > lower)) jpq_offer(&cq, old[s]);
          free(old);
        }
        if (cq.n < ccap) jpq_offer(&cq, it);
        if (nn == item) continue; /* :607-609 */
        jpq_offer(wq, it);
        if (wq->n > ef) jpq_poll(wq);
        lower = wq->a[0].d;
      }
    }
  }
  free(cq.a);
}

/* bestEntryPointUntilLayer (:447-475) from the entry point down to layer top + 1 */
static int64_t descend(const hbuild *g, int64_t item, int top) {
  int64_t cur = g->entry;
  if (top < g->max_level) {
    float cur_dist = item_distance(g, item, cur);
    for (int level = g->max_level; level > top; level--) {
      int changed = 1;
      while (changed) {
        changed = 0;
        const int64_t *list;
        int ln = list_of(g, level, cur, &list);
        for (int j = 0; j < ln; j++) {
          float t = item_distance(g, item, list[j]);
          if (t < cur_dist) { cur_dist = t; cur = list[j]; changed = 1; }
        }
      }
    }
  }
  return cur;
}

static int holds(const hbuild *g, int level, int64_t base, int64_t item) {
  const int64_t *conn;
  int cn = list_of(g, level, base, &conn);
  for (int i = 0; i < cn; i++) if (conn[i] == item) return 1;
  return 0;
}

/* ---- the unbatched reInsert (:226-329) ---- */
static void reinsert(hbuild *g, int64_t item, int ccap, uint8_t *visited, uint8_t *mark, int64_t *sc, ustats *st) {
  if (g->entry < 0) return;                 /* :231-233 checkState(entryPoint.isPresent) */
  const int cur_level = top_of(g, item);    /* :236-250 (and :239-240: HnswNode(0, item) must exist) */
  if (cur_level < 0) return;
  int64_t *neigh = malloc(sizeof(int64_t) * (size_t)(g->cap + 1));
  int64_t *upd = malloc(sizeof(int64_t) * (size_t)(g->cap + 1));
  for (int layer = 0; layer <= cur_level; layer++) { /* :254-324 */
    const int64_t *one;
    const int c1 = list_of(g, layer, item, &one);
    if (c1 == 0) continue;
    const int s = set_cand(g, layer, item, sc, mark);
    int64_t *hop = malloc(sizeof(int64_t) * (size_t)c1);
    memcpy(hop, one, sizeof(int64_t) * (size_t)c1);
    for (int i = 0; i < c1; i++) {
      if (hop[i] == item) continue;
      const int nk = propose(g, layer, hop[i], sc, s, neigh);
      put_list(g, layer, hop[i], neigh, nk); /* setConnectionList(neigh, layer, neighbours) */
      st->n_relinks++;
    }
    free(hop);
  }
  /* :328 wireConnectionForAllLayers(entryPoint, item, curLevel, maxLevelCopy, true) */
  int64_t cur = descend(g, item, cur_level);
  for (int level = imin(cur_level, g->max_level); level >= 0; level--) {
    jpq wq;
    search_layer_update(g, item, cur, g->efc, level, visited, &wq, ccap);
    /* mutuallyConnectNewElement(item, candidates, level, true), :384-440 */
    const int nn = select_by_heuristic(g, &wq, item, g->max_m, neigh);
    free(wq.a);
    if (nn == 0) { st->n_kept++; cur = item; continue; } /* (the reference throws at :439) */
    put_list(g, level, item, neigh, nn);
    const int M = level == 0 ? g->max_m0 : g->max_m;
    for (int i = 0; i < nn; i++) {
      const int64_t other = neigh[i];
      if (other == item) continue;
      if (holds(g, level, other, item)) { st->n_present++; continue; } /* :405-412 */
      const int64_t *conn;
      int cn = list_of(g, level, other, &conn);
      if (cn < M) {
        memcpy(upd, conn, sizeof(int64_t) * (size_t)cn);
        upd[cn] = item;
        put_list(g, level, other, upd, cn + 1);
      } else {
        jpq q;
        jpq_init(&q, 0);
        for (int j = 0; j < cn; j++) { qitem it = {item_distance(g, other, conn[j]), conn[j]}; jpq_offer(&q, it); }
        qitem it = {item_distance(g, other, item), item};
        jpq_offer(&q, it);
        int un = select_by_heuristic(g, &q, other, M, upd);
        put_list(g, level, other, upd, un);
        free(q.a);
      }
    }
    cur = neigh[0];
  }
  free(neigh);
  free(upd);
}

/* ---- the device's rounds ---- */
typedef struct { int level; int64_t v; int n; int64_t *list; } proposal;

static void update_round(hbuild *g, const int64_t *items, int64_t m, int ccap, int link_cap, uint8_t *visited, uint8_t *mark,
                         int64_t *sc, int32_t **stamp, int32_t round_id, ustats *st) {
  int *tops = malloc(sizeof(int) * (size_t)m);
  for (int64_t t = 0; t < m; t++) tops[t] = top_of(g, items[t]);
  /* ---- 2: every proposal against the graph as the round found it, then in request order (the latest wins) ---- */
  int64_t np = 0, pcap = 64;
  proposal *props = malloc(sizeof(proposal) * (size_t)pcap);
  for (int64_t t = 0; t < m; t++) {
    const int64_t u = items[t];
    for (int layer = 0; layer <= tops[t]; layer++) {
      const int64_t *one;
      const int c1 = list_of(g, layer, u, &one);
      if (c1 == 0) continue;
      const int s = set_cand(g, layer, u, sc, mark);
      for (int i = 0; i < c1; i++) {
        if (one[i] == u) continue;
        if (np == pcap) { pcap *= 2; props = realloc(props, sizeof(proposal) * (size_t)pcap); }
        proposal *p = &props[np++];
        p->level = layer;
        p->v = one[i];
        p->list = malloc(sizeof(int64_t) * (size_t)(g->cap + 1));
        p->n = propose(g, layer, one[i], sc, s, p->list);
      }
    }
  }
  for (int64_t i = 0; i < np; i++) {
    proposal *p = &props[i];
    if (stamp[p->level][p->v] == round_id) st->n_superseded++;
    stamp[p->level][p->v] = round_id;
    put_list(g, p->level, p->v, p->list, p->n);
    free(p->list);
    st->n_relinks++;
  }
  free(props);
  /* ---- 3: the walks; own lists aside, back links recorded ---- */
  int64_t nl = 0, lcap = 64;
  backlink *links = malloc(sizeof(backlink) * (size_t)lcap);
  int64_t **own = malloc(sizeof(int64_t *) * (size_t)m);
  int **own_n = malloc(sizeof(int *) * (size_t)m);
  for (int64_t t = 0; t < m; t++) {
    own[t] = NULL;
    own_n[t] = NULL;
    const int64_t u = items[t];
    if (tops[t] < 0) continue;
    own[t] = malloc(sizeof(int64_t) * (size_t)(tops[t] + 1) * (size_t)(g->cap + 1));
    own_n[t] = malloc(sizeof(int) * (size_t)(tops[t] + 1));
    int64_t cur = descend(g, u, tops[t]);
    for (int level = imin(tops[t], g->max_level); level >= 0; level--) {
      jpq wq;
      search_layer_update(g, u, cur, g->efc, level, visited, &wq, ccap);
      int64_t *neigh = own[t] + (size_t)level * (size_t)(g->cap + 1);
      const int nn = select_by_heuristic(g, &wq, u, g->max_m, neigh);
      free(wq.a);
      own_n[t][level] = nn;
      if (nn == 0) { st->n_kept++; cur = u; continue; }
      for (int e = 0; e < nn; e++) {
        if (nl == lcap) { lcap *= 2; links = realloc(links, sizeof(backlink) * (size_t)lcap); }
        links[nl].level = level; links[nl].target = neigh[e]; links[nl].t = t; nl++;
      }
      cur = neigh[0];
    }
  }
  for (int64_t t = 0; t < m; t++) {
    if (!own[t]) continue;
    for (int level = 0; level <= tops[t]; level++)
      if (own_n[t][level] > 0) put_list(g, level, items[t], own[t] + (size_t)level * (size_t)(g->cap + 1), own_n[t][level]);
    free(own[t]);
    free(own_n[t]);
  }
  free(own);
  free(own_n);
  /* ---- 4: phase B; an addition the list already holds is dropped ---- */
  qsort(links, (size_t)nl, sizeof(backlink), backlink_cmp);
  int64_t *adds = malloc(sizeof(int64_t) * (size_t)(nl > 0 ? nl : 1));
  int64_t *tid = malloc(sizeof(int64_t) * (size_t)link_cap), *cid = malloc(sizeof(int64_t) * (size_t)link_cap);
  float *td = malloc(sizeof(float) * (size_t)link_cap), *cd = malloc(sizeof(float) * (size_t)link_cap);
  int64_t *upd = malloc(sizeof(int64_t) * (size_t)(g->cap + 1));
  for (int64_t i0 = 0; i0 < nl;) {
    int64_t i1 = i0;
    while (i1 < nl && links[i1].level == links[i0].level && links[i1].target == links[i0].target) i1++;
    const int level = links[i0].level;
    const int64_t base = links[i0].target;
    const int M = level == 0 ? g->max_m0 : g->max_m;
    const int64_t *conn;
    const int old_n = list_of(g, level, base, &conn);
    int add_n = 0;
    for (int64_t e = i0; e < i1; e++) {
      const int64_t it = items[links[e].t];
      if (holds(g, level, base, it)) st->n_present++;
      else adds[add_n++] = it;
    }
    if (add_n > 0 && old_n + add_n <= M) {
      if (old_n > 0) memcpy(upd, conn, sizeof(int64_t) * (size_t)old_n);
      for (int e = 0; e < add_n; e++) upd[old_n + e] = adds[e];
      put_list(g, level, base, upd, old_n + add_n);
    } else if (add_n > 0) {
      int cn = old_n + add_n;
      if (cn > link_cap) cn = link_cap;
      for (int i = 0; i < cn; i++) {
        tid[i] = i < old_n ? conn[i] : adds[i - old_n];
        td[i] = item_distance(g, base, tid[i]);
      }
      for (int i = 0; i < cn; i++) {
        int rank = 0;
        for (int e = 0; e < cn; e++) {
          int c = jfloat_compare(td[e], td[i]);
          rank += (c < 0 || (c == 0 && e < i)) ? 1 : 0;
        }
        cid[rank] = tid[i];
        cd[rank] = td[i];
      }
      int nk = 0;
      for (int i = 0; i < cn && nk < M; i++) {
        if (cid[i] == base) continue;
        int include = 1;
        for (int k = 0; k < nk; k++)
          if (item_distance(g, upd[k], cid[i]) < cd[i]) { include = 0; break; }
        if (include) upd[nk++] = cid[i];
      }
      put_list(g, level, base, upd, nk);
    }
    i0 = i1;
  }
  free(adds); free(tid); free(cid); free(td); free(cd); free(upd); free(links); free(tops);
}

/* x: the stored rows before the update (fp16-rounded, as the index holds them), [n][d]; rows: the stored form of the updated
 * rows [n_upd][d]; pos: their positions in request order.  The graph in and out as oracle_hnsw_search reads it (out: entries
 * sorted by (level, item)).  batch = 0: the unbatched reInsert sequence.  stats: relinks, superseded, additions already present,
 * lists kept.  Returns the number of entries, -1 if the output arrays are too small. */
int64_t ref_hnsw_update(int32_t metric, int64_t n, int32_t d, const float *x, int32_t max_m, int32_t ef_construction,
                        int64_t entry_point, int32_t max_level, int64_t n_entries, const int32_t *entry_level,
                        const int64_t *entry_item, const int64_t *entry_offsets, const int64_t *entry_neighbours, int64_t n_upd,
                        const float *rows, const int64_t *pos, int32_t batch, int32_t ccap, int32_t link_cap, int64_t cap_entries,
                        int64_t cap_neighbours, int32_t *out_level, int64_t *out_item, int64_t *out_offsets,
                        int64_t *out_neighbours, int64_t *out_entry_point, int32_t *out_max_level, int64_t *stats) {
  hbuild g;
  float *xw = malloc(sizeof(float) * (size_t)(n > 0 ? n : 1) * (size_t)d);
  memcpy(xw, x, sizeof(float) * (size_t)n * (size_t)d);
  g.n = n; g.metric = metric; g.d = d; g.max_m = max_m; g.max_m0 = 2 * max_m; g.efc = ef_construction; g.x = xw;
  g.cap = 2 * max_m + 1;
  g.entry = entry_point; g.max_level = max_level;
  int top = max_level > 0 ? max_level : 0;
  for (int64_t e = 0; e < n_entries; e++) if (entry_level[e] > top) top = entry_level[e];
  g.n_levels = top + 1;
  g.cnt = malloc(sizeof(int32_t *) * (size_t)g.n_levels);
  g.nb = malloc(sizeof(int64_t *) * (size_t)g.n_levels);
  int32_t **stamp = malloc(sizeof(int32_t *) * (size_t)g.n_levels);
  for (int l = 0; l < g.n_levels; l++) {
    g.cnt[l] = malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    stamp[l] = malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    for (int64_t i = 0; i < n; i++) { g.cnt[l][i] = -1; stamp[l][i] = -1; }
    g.nb[l] = malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1) * (size_t)g.cap);
  }
  for (int64_t e = 0; e < n_entries; e++) {
    const int64_t c = entry_offsets[e + 1] - entry_offsets[e];
    put_list(&g, entry_level[e], entry_item[e], entry_neighbours + entry_offsets[e], (int)c);
  }
  uint8_t *visited = malloc((size_t)(n > 0 ? n : 1));
  uint8_t *mark = calloc((size_t)(n > 0 ? n : 1), 1);
  int64_t *sc = malloc(sizeof(int64_t) * (size_t)(1 + g.max_m0 + g.max_m0 * g.max_m0));
  ustats st = {0, 0, 0, 0};
  int64_t rounds = 0;
  if (batch <= 0) {
    for (int64_t k = 0; k < n_upd; k++) {
      memcpy(xw + (size_t)pos[k] * d, rows + (size_t)k * d, sizeof(float) * (size_t)d);
      reinsert(&g, pos[k], ccap, visited, mark, sc, &st);
    }
    rounds = n_upd;
  } else {
    for (int64_t r0 = 0; r0 < n_upd; r0 += batch) {
      const int64_t m = n_upd - r0 < batch ? n_upd - r0 : batch;
      for (int64_t k = r0; k < r0 + m; k++) memcpy(xw + (size_t)pos[k] * d, rows + (size_t)k * d, sizeof(float) * (size_t)d);
      if (g.entry >= 0) update_round(&g, pos + r0, m, ccap, link_cap, visited, mark, sc, stamp, (int32_t)rounds, &st);
      rounds++;
    }
  }
  int64_t ne = 0, nnb = 0;
  int fits = 1;
  for (int l = 0; l < g.n_levels && fits; l++)
    for (int64_t i = 0; i < n; i++) {
      if (g.cnt[l][i] < 0) continue;
      if (ne >= cap_entries || nnb + g.cnt[l][i] > cap_neighbours) { fits = 0; break; }
      out_level[ne] = l;
      out_item[ne] = i;
      out_offsets[ne] = nnb;
      memcpy(out_neighbours + nnb, g.nb[l] + (size_t)i * g.cap, sizeof(int64_t) * (size_t)g.cnt[l][i]);
      nnb += g.cnt[l][i];
      ne++;
    }
  if (fits) out_offsets[ne] = nnb;
  *out_entry_point = g.entry;
  *out_max_level = g.max_level;
  stats[0] = rounds; stats[1] = st.n_relinks; stats[2] = st.n_superseded; stats[3] = st.n_present; stats[4] = st.n_kept;
  for (int l = 0; l < g.n_levels; l++) { free(g.cnt[l]); free(g.nb[l]); free(stamp[l]); }
  free(g.cnt); free(g.nb); free(stamp); free(visited); free(mark); free(sc); free(xw);
  return fits ? ne : -1;
}
