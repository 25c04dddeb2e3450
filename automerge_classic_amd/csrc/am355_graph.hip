// Hash-graph queries of the C ABI over the changes a context has applied (include/am355.h: am355_find_changes, am355_changes_since,
// am355_changes_added, am355_missing_deps): what BackendDoc.getChangeByHash / getChanges / getChangesAdded / getMissingDeps answer
// from changeIndexByHash, dependenciesByHash and dependentsByHash (new.js:1921-2028), answered from the engine's own tables as lists
// of indexes into its list of changes.
//
// Two halves. The TRAVERSALS run on the host over indexes: their order is sequential by definition (a stack, popped from its end)
// and they visit what is new, which is short in the usual case. The MEMBERSHIP TESTS are what grows with the document -- is this hash
// an applied change, which of my changes does the other state lack -- and go to the device from graph_probe_min probes on: the
// context's hashes are in HBM already (d_hashes), so a query uploads the foreign hashes only. Below that the host index answers; both
// give the same indexes (tests/test_hash_graph.py runs every case both ways).
//
// No call here changes the replayed state: they read h_hashes / d_hashes, applied_change, pending_change, heads and the dependency
// records, and write the members of am355_ctx::graph, d_hash_tab (which no resident call reads and every full replay builds anew),
// d_graph and h_graph.
//
// Included at the end of am355_calls.hip, not compiled by itself.
#include "am355_ctx.h"

namespace am355 {

// One thread per change [first, n): claims the first free slot from hash_slot on. The same hash twice: the slot keeps the smaller index.
// (A table holds at most half as many changes as it has slots, so a free slot is always found; the bound only ends a walk over a
// table somebody filled wrongly.)
__global__ __launch_bounds__(BLOCK) void k_graph_insert(const uint8_t* __restrict__ hashes, uint32_t first, uint32_t n, uint32_t* __restrict__ tab, uint32_t mask) {
  const uint32_t c = first + gtid();
  if (c >= n || c < first) return;
  const uint8_t* h = hashes + 32 * (size_t)c;
  uint32_t i = hash_slot(h, mask);
  for (uint32_t probes = 0; probes <= mask; probes++) {
    const uint32_t old = atomicCAS(&tab[i], 0u, c + 1);
    if (old == 0) return;
    if (equal32(hashes + 32 * (size_t)(old - 1), h)) { atomicMin(&tab[i], c + 1); return; }
    i = (i + 1) & mask;
  }
}

// the change index `h` stands under in the table over `hashes`, or NONE32
__device__ __forceinline__ uint32_t graph_find(const uint8_t* __restrict__ hashes, const uint32_t* __restrict__ tab, uint32_t mask, const uint8_t* h) {
  uint32_t i = hash_slot(h, mask);
  for (uint32_t probes = 0; probes <= mask; probes++) {
    const uint32_t v = tab[i];
    if (v == 0) return NONE32;
    if (equal32(hashes + 32 * (size_t)(v - 1), h)) return v - 1;
    i = (i + 1) & mask;
  }
  return NONE32;
}

// One thread per query: out[q] = index of the change with hash queries[q] in the table over `hashes`, or NONE32.
__global__ __launch_bounds__(BLOCK) void k_hash_probe(const uint8_t* __restrict__ hashes, const uint32_t* __restrict__ tab, uint32_t mask,
                                                      const uint8_t* __restrict__ queries, uint32_t n_queries, uint32_t* __restrict__ out) {
  const uint32_t q = gtid();
  if (q >= n_queries) return;
  out[q] = graph_find(hashes, tab, mask, queries + 32 * (size_t)q);
}

// One thread per change of the context: is its hash missing from the table over `other`? One 64-bit word per wavefront, bit = lane
// (every lane reaches the ballot: no early return; lanes past n vote 0).
__global__ __launch_bounds__(BLOCK) void k_absent_ballot(const uint8_t* __restrict__ other, const uint32_t* __restrict__ tab, uint32_t mask,
                                                         const uint8_t* __restrict__ hashes, uint32_t n, unsigned long long* __restrict__ words, uint32_t n_words) {
  const uint32_t i = gtid();
  bool absent = false;
  if (i < n) absent = graph_find(other, tab, mask, hashes + 32 * (size_t)i) == NONE32;
  const unsigned long long b = __ballot(absent ? 1 : 0);
  const uint32_t w = i >> 6;
  if ((threadIdx.x & (WAVE - 1)) == 0 && w < n_words) words[w] = b;
}

}  // namespace am355

namespace {

constexpr uint32_t MAX_TABLE_CHANGES = 0x3fffffffu;   // (2 n + 64 slots must fit 32 bits)

uint32_t table_mask_for(uint32_t n) { return pow2_at_least(2 * (uint64_t)n + 64) - 1; }
size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }
uint32_t blocks_for(uint32_t n) { return (n + BLOCK - 1) / BLOCK; }

// ---- host index: hash -> staged index of the applied change ------------------------------------------------------------------
uint64_t host_key(const uint8_t* h) { uint64_t v; memcpy(&v, h, 8); return (v * 0x9e3779b97f4a7c15ull) >> 20; }
void host_add(std::vector<uint32_t>& t, const uint8_t* hs, uint32_t ci) {
  const size_t mask = t.size() - 1;
  size_t i = (size_t)host_key(hs + 32 * (size_t)ci) & mask;
  while (t[i]) i = (i + 1) & mask;
  t[i] = ci + 1;
}
uint32_t host_find(const std::vector<uint32_t>& t, const uint8_t* hs, const uint8_t* h) {
  if (t.empty()) return NONE32;
  const size_t mask = t.size() - 1;
  for (size_t i = (size_t)host_key(h) & mask; t[i]; i = (i + 1) & mask)
    if (memcmp(hs + 32 * (size_t)(t[i] - 1), h, 32) == 0) return t[i] - 1;
  return NONE32;
}

std::string hex_of(const uint8_t* h) {
  static const char* d = "0123456789abcdef";
  std::string s(64, '0');
  for (int k = 0; k < 32; k++) { s[2 * k] = d[h[k] >> 4]; s[2 * k + 1] = d[h[k] & 15]; }
  return s;
}

int served(am355_ctx* c, const char* what) {
  if (!c->staged || !c->replayed || c->is_document || !c->h_hashes.p) return fail(c, AM355_E_STATE, "%s: a replayed state of changes is needed", what);
  if (c->shard_world > 1) return fail(c, AM355_E_UNSUPPORTED, "%s on a sharded context", what);
  if (c->n_changes > MAX_TABLE_CHANGES) return fail(c, AM355_E_UNSUPPORTED, "%s: more than 2^30 changes", what);
  return AM355_OK;
}

// the dependents CSR over the first g.n_applied applied entries, by one counting pass; the chains are folded in
void build_dependents(am355_ctx* c) {
  am355_ctx::GraphIndex& g = c->graph;
  const uint32_t n = g.n_staged;
  g.dpt_first.assign((size_t)n + 1, 0);
  for (uint32_t a = 0; a < g.n_applied; a++) {
    const uint32_t i = c->applied_change[a];
    for (uint32_t k = g.dep_first[i]; k < g.dep_first[i + 1]; k++)
      if (g.dep_index[k] < n) g.dpt_first[g.dep_index[k] + 1]++;
  }
  for (uint32_t i = 0; i < n; i++) g.dpt_first[i + 1] += g.dpt_first[i];
  g.dpt_index.resize(g.dpt_first[n]);
  std::vector<uint32_t> at(g.dpt_first.begin(), g.dpt_first.end() - 1);
  for (uint32_t a = 0; a < g.n_applied; a++) {
    const uint32_t i = c->applied_change[a];
    for (uint32_t k = g.dep_first[i]; k < g.dep_first[i + 1]; k++)
      if (g.dep_index[k] < n) g.dpt_index[at[g.dep_index[k]]++] = i;
  }
  g.dpt_applied = g.n_applied;
  g.chain_head.assign(n, NONE32);
  g.chain_tail.assign(n, NONE32);
  g.chain_child.clear();
  g.chain_next.clear();
}

// Brings c->graph up to the applied changes of the context: extended when the applied list has only grown since the last query (the
// batches of resident calls: their dependency records are res_dep_*), rebuilt when a replay made the list anew.
int ensure_index(am355_ctx* c) {
  am355_ctx::GraphIndex& g = c->graph;
  const uint32_t n = c->n_changes, na = (uint32_t)c->applied_change.size();
  const uint8_t* hs = c->h_hashes.as<uint8_t>();
  if (g.epoch == c->graph_epoch && g.n_staged == n && g.n_applied == na) return AM355_OK;
  bool extend = g.epoch == c->graph_epoch && g.n_staged <= n && g.n_applied <= na && g.n_staged >= c->res_dep_base && c->pending_change.empty() && na == n &&
                g.n_applied == g.n_staged && 4 * (size_t)n + 64 <= g.table.size();
  if (extend)
    for (uint32_t i = g.n_staged; extend && i < n; i++) {
      const uint32_t j = i - c->res_dep_base;
      extend = c->applied_change[i] == i && j + 1 < c->res_dep_first.size();
    }
  if (extend) {
    g.is_applied.resize(n, 1);
    g.chain_head.resize(n, NONE32);
    g.chain_tail.resize(n, NONE32);
    for (uint32_t i = g.n_staged; i < n; i++) {
      const uint32_t j = i - c->res_dep_base;
      for (uint32_t k = c->res_dep_first[j]; k < c->res_dep_first[j + 1]; k++) {
        const uint32_t d = c->res_dep_index[k];
        if (d >= i) return fail(c, AM355_E_DEVICE, "internal: dependency record of an appended change names a later change");
        g.dep_index.push_back(d);
        // (new.js:1853-1856: the change is pushed onto the list of every dependency, in the order of its deps)
        const uint32_t e = (uint32_t)g.chain_child.size();
        g.chain_child.push_back(i);
        g.chain_next.push_back(NONE32);
        if (g.chain_tail[d] == NONE32) g.chain_head[d] = e; else g.chain_next[g.chain_tail[d]] = e;
        g.chain_tail[d] = e;
      }
      g.dep_first.push_back((uint32_t)g.dep_index.size());
      host_add(g.table, hs, i);
    }
    g.n_staged = n;
    g.n_applied = na;
    if (g.chain_child.size() > g.dpt_index.size() + 1024) build_dependents(c);
    return AM355_OK;
  }
  // anew: the dependency indexes the device resolved (am355_get_dep_graph), the applied changes' hashes into the host index
  static const uint32_t none[1] = {0};
  const uint32_t *first = none, *index = none;
  if (n) {
    int rc = get_dep_graph_impl(c, &first, &index, nullptr);
    if (rc) return rc;
  }
  g.epoch = ~0ull;
  g.is_applied.assign(n, 0);
  size_t cap = 64;
  while (cap < 8 * (size_t)n + 64) cap <<= 1;   // (room to double before the index is rebuilt)
  g.table.assign(cap, 0);
  for (uint32_t a = 0; a < na; a++) {
    const uint32_t i = c->applied_change[a];
    if (i >= n) return fail(c, AM355_E_DEVICE, "internal: applied change index out of range");
    g.is_applied[i] = 1;
    host_add(g.table, hs, i);
  }
  g.dep_first.assign(first, first + n + 1);
  g.dep_index.assign(index, index + first[n]);
  // a dependency the device resolved to another copy of the same change (a batch with duplicates) or to a queued change: the
  // applied change with that hash, if there is one
  for (uint32_t& d : g.dep_index)
    if (d != NONE32 && (d >= n || !g.is_applied[d])) d = d < n ? host_find(g.table, hs, hs + 32 * (size_t)d) : NONE32;
  g.n_staged = n;
  g.n_applied = na;
  build_dependents(c);
  g.epoch = c->graph_epoch;
  return AM355_OK;
}

// d_hash_tab over the staged changes [0, n) of this replay: built anew, or the changes staged since inserted. Enqueues on c->stream.
int ensure_device_table(am355_ctx* c) {
  am355_ctx::GraphIndex& g = c->graph;
  const uint32_t n = c->n_changes;
  int rc = flush_uploads(c);   // (the hashes of a resident batch may still be queued for d_hashes)
  if (rc) return rc;
  if (!c->d_hashes.p || c->d_hashes.cap < 32 * (size_t)n) return fail(c, AM355_E_STATE, "the context's hashes are not in device memory");
  hipStream_t st = c->stream;
  const bool extend = g.tab_epoch == c->graph_epoch && g.tab_n <= n && 2 * (uint64_t)n + 64 <= (uint64_t)g.tab_mask + 1 && c->d_hash_tab.cap >= 4 * ((size_t)g.tab_mask + 1);
  uint32_t first = g.tab_n;
  if (!extend) {
    g.tab_epoch = ~0ull;
    g.tab_mask = pow2_at_least(4 * (uint64_t)n + 64) - 1;   // (as the host index: room to double)
    if (!c->d_hash_tab.ensure(4 * ((size_t)g.tab_mask + 1))) return fail(c, AM355_E_NOMEM, "device allocation failed");
    HIPCHK(c, hipMemsetAsync(c->d_hash_tab.p, 0, 4 * ((size_t)g.tab_mask + 1), st));
    first = 0;
  }
  if (n > first) AM355_LAUNCH_INDEPENDENT(k_graph_insert, dim3(blocks_for(n - first)), dim3(BLOCK), st, (const uint8_t*)c->d_hashes.as<uint8_t>(), first, n, c->d_hash_tab.as<uint32_t>(), g.tab_mask);
  g.tab_n = n;
  g.tab_epoch = c->graph_epoch;
  return AM355_OK;
}

// out[k] = staged index of the APPLIED change with hash hashes[k], or NONE32 (a queued change does not count: new.js:1999-2002 reads
// changeIndexByHash). n at or above graph_probe_min: probed on the device.
int lookup(am355_ctx* c, const uint8_t* hashes, uint32_t n, uint32_t* out) {
  am355_ctx::GraphIndex& g = c->graph;
  const uint8_t* hs = c->h_hashes.as<uint8_t>();
  if (!n) return AM355_OK;
  if (n < c->graph_probe_min || c->graph_probe_min == 0xffffffffu || !c->n_changes) {
    for (uint32_t k = 0; k < n; k++) out[k] = host_find(g.table, hs, hashes + 32 * (size_t)k);
    c->n_graph_host++;
    return AM355_OK;
  }
  int rc = ensure_device_table(c);
  if (rc) return rc;
  const size_t o_out = round256(32 * (size_t)n);
  if (!c->d_graph.ensure(o_out + round256(4 * (size_t)n)) || !c->h_graph.ensure(4 * (size_t)n)) return fail(c, AM355_E_NOMEM, "allocation failed");
  hipStream_t st = c->stream;
  uint8_t* d = c->d_graph.as<uint8_t>();
  HIPCHK(c, hipMemcpyAsync(d, hashes, 32 * (size_t)n, hipMemcpyHostToDevice, st));
  AM355_LAUNCH_INDEPENDENT(k_hash_probe, dim3(blocks_for(n)), dim3(BLOCK), st, (const uint8_t*)c->d_hashes.as<uint8_t>(), (const uint32_t*)c->d_hash_tab.as<uint32_t>(), g.tab_mask,
                           (const uint8_t*)d, n, (uint32_t*)(d + o_out));
  HIPCHK(c, hipMemcpyAsync(c->h_graph.p, d + o_out, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const uint32_t* found = c->h_graph.as<uint32_t>();
  for (uint32_t k = 0; k < n; k++) {
    uint32_t i = found[k];
    if (i != NONE32 && (i >= g.n_staged || !g.is_applied[i])) i = host_find(g.table, hs, hashes + 32 * (size_t)k);   // (the table holds queued changes and second copies too)
    out[k] = i;
  }
  c->n_graph_device++;
  return AM355_OK;
}

template <class F>
void for_dependents(const am355_ctx::GraphIndex& g, uint32_t i, F f) {
  if ((size_t)i + 1 < g.dpt_first.size())   // (a change applied since the CSR was built has chains only)
    for (uint32_t k = g.dpt_first[i]; k < g.dpt_first[i + 1]; k++) f(g.dpt_index[k]);
  for (uint32_t e = g.chain_head[i]; e != NONE32; e = g.chain_next[e]) f(g.chain_child[e]);
}

}  // namespace

int find_changes_impl(am355_ctx* c, const uint8_t* hashes, uint32_t n, uint32_t* out_idx) {
  if (!c || (n && (!hashes || !out_idx))) return c ? fail(c, AM355_E_ARG, "null argument") : AM355_E_ARG;
  int rc = served(c, "am355_find_changes");
  if (rc) return rc;
  (void)hipSetDevice(c->device);
  if (!n) return AM355_OK;
  rc = ensure_index(c);
  if (rc) return rc;
  return lookup(c, hashes, n, out_idx);
}

// BackendDoc.getChanges(haveDeps), new.js:1921-1976, over indexes
int changes_since_impl(am355_ctx* c, const uint8_t* have, uint32_t n_have, const uint32_t** idx, uint32_t* n_out) {
  if (!c || !idx || !n_out || (n_have && !have)) return c ? fail(c, AM355_E_ARG, "null argument") : AM355_E_ARG;
  int rc = served(c, "am355_changes_since");
  if (rc) return rc;
  (void)hipSetDevice(c->device);
  am355_ctx::GraphIndex& g = c->graph;
  std::vector<uint32_t>& out = g.out_idx;
  out.clear();
  auto done = [&]() { *idx = out.data(); *n_out = (uint32_t)out.size(); return AM355_OK; };
  if (n_have == 0) {   // :1925-1927: everything, in application order
    out.assign(c->applied_change.begin(), c->applied_change.end());
    return done();
  }
  rc = ensure_index(c);
  if (rc) return rc;
  std::vector<uint32_t> have_idx(n_have);
  rc = lookup(c, have, n_have, have_idx.data());
  if (rc) return rc;
  // :1930-1936 (the first hash without a list of dependents ends the call)
  for (uint32_t k = 0; k < n_have; k++)
    if (have_idx[k] == NONE32) return fail(c, AM355_E_INVALID, "hash not found: %s", hex_of(have + 32 * (size_t)k).c_str());
  const uint8_t* hs = c->h_hashes.as<uint8_t>();
  std::vector<uint8_t> seen(g.n_staged, 0);
  std::vector<uint32_t> stack;
  for (uint32_t k = 0; k < n_have; k++) {
    seen[have_idx[k]] = 1;
    for_dependents(g, have_idx[k], [&](uint32_t d) { stack.push_back(d); });
  }
  // :1938-1950: forward over the dependents, given up at a change with a dependency not seen yet
  while (!stack.empty()) {
    const uint32_t i = stack.back();
    stack.pop_back();
    seen[i] = 1;
    out.push_back(i);
    bool all = true;
    for (uint32_t k = g.dep_first[i]; all && k < g.dep_first[i + 1]; k++) all = g.dep_index[k] < g.n_staged && seen[g.dep_index[k]];
    if (!all) break;
    for_dependents(g, i, [&](uint32_t d) { stack.push_back(d); });
  }
  // :1952-1956
  bool complete = stack.empty();
  for (size_t k = 0; complete && k < c->heads.size() / 32; k++) {
    const uint32_t h = host_find(g.table, hs, &c->heads[32 * k]);
    complete = h != NONE32 && seen[h];
  }
  if (complete) return done();
  // :1958-1972: everything that is not an ancestor of haveDeps, in application order
  std::fill(seen.begin(), seen.end(), 0);
  stack.assign(have_idx.begin(), have_idx.end());
  while (!stack.empty()) {
    const uint32_t i = stack.back();
    stack.pop_back();
    if (seen[i]) continue;
    for (uint32_t k = g.dep_first[i]; k < g.dep_first[i + 1]; k++) {
      if (g.dep_index[k] >= g.n_staged) return fail(c, AM355_E_DEVICE, "internal: an applied change has a dependency that is not applied");
      stack.push_back(g.dep_index[k]);
    }
    seen[i] = 1;
  }
  out.clear();
  for (uint32_t i : c->applied_change)
    if (!seen[i]) out.push_back(i);
  return done();
}

// BackendDoc(ctx).getChangesAdded(other), new.js:1979-1997: `other` = the hashes of the changes the other state has applied
int changes_added_impl(am355_ctx* c, const uint8_t* other, uint32_t n_other, const uint32_t** idx, uint32_t* n_out) {
  if (!c || !idx || !n_out || (n_other && !other)) return c ? fail(c, AM355_E_ARG, "null argument") : AM355_E_ARG;
  int rc = served(c, "am355_changes_added");
  if (rc) return rc;
  if (n_other > MAX_TABLE_CHANGES) return fail(c, AM355_E_UNSUPPORTED, "am355_changes_added: more than 2^30 hashes");
  (void)hipSetDevice(c->device);
  am355_ctx::GraphIndex& g = c->graph;
  std::vector<uint32_t>& out = g.out_idx;
  out.clear();
  auto done = [&]() { *idx = out.data(); *n_out = (uint32_t)out.size(); return AM355_OK; };
  const uint32_t n = c->n_changes;
  if (!n || c->applied_change.empty()) return done();
  rc = ensure_index(c);
  if (rc) return rc;
  const uint8_t* hs = c->h_hashes.as<uint8_t>();
  // membership: one probe per change of this context
  const bool device = n_other != 0 && c->graph_probe_min != 0xffffffffu && n >= c->graph_probe_min;
  std::vector<uint32_t> other_tab;
  if (device) {
    rc = flush_uploads(c);
    if (rc) return rc;
    if (!c->d_hashes.p || c->d_hashes.cap < 32 * (size_t)n) return fail(c, AM355_E_STATE, "the context's hashes are not in device memory");
    const uint32_t mask = table_mask_for(n_other), n_words = (n + 63) / 64;
    const size_t o_tab = round256(32 * (size_t)n_other), o_words = o_tab + round256(4 * ((size_t)mask + 1));
    if (!c->d_graph.ensure(o_words + round256(8 * (size_t)n_words)) || !c->h_graph.ensure(8 * (size_t)n_words)) return fail(c, AM355_E_NOMEM, "allocation failed");
    hipStream_t st = c->stream;
    uint8_t* d = c->d_graph.as<uint8_t>();
    HIPCHK(c, hipMemcpyAsync(d, other, 32 * (size_t)n_other, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d + o_tab, 0, 4 * ((size_t)mask + 1), st));
    AM355_LAUNCH_INDEPENDENT(k_graph_insert, dim3(blocks_for(n_other)), dim3(BLOCK), st, (const uint8_t*)d, 0u, n_other, (uint32_t*)(d + o_tab), mask);
    hipLaunchKernelGGL(k_absent_ballot, dim3(blocks_for(n)), dim3(BLOCK), 0, st, (const uint8_t*)d, (const uint32_t*)(d + o_tab), mask, (const uint8_t*)c->d_hashes.as<uint8_t>(), n,
                       (unsigned long long*)(d + o_words), n_words);
    HIPCHK(c, hipMemcpyAsync(c->h_graph.p, d + o_words, 8 * (size_t)n_words, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    g.absent.assign(c->h_graph.as<uint64_t>(), c->h_graph.as<uint64_t>() + n_words);
    c->n_graph_device++;
  } else {
    if (n_other) {
      size_t cap = 64;
      while (cap < 2 * (size_t)n_other + 64) cap <<= 1;
      other_tab.assign(cap, 0);
      for (uint32_t k = 0; k < n_other; k++)
        if (host_find(other_tab, other, other + 32 * (size_t)k) == NONE32) host_add(other_tab, other, k);
      c->n_graph_host++;
    }
  }
  auto absent = [&](uint32_t i) {
    if (device) return ((g.absent[i >> 6] >> (i & 63)) & 1) != 0;
    return host_find(other_tab, other, hs + 32 * (size_t)i) == NONE32;
  };
  // :1984-1992: depth first from the heads through the dependencies, stopping at what `other` holds
  std::vector<uint8_t> seen(g.n_staged, 0);
  std::vector<uint32_t> stack;
  for (size_t k = 0; k < c->heads.size() / 32; k++) {
    const uint32_t h = host_find(g.table, hs, &c->heads[32 * k]);
    if (h == NONE32) return fail(c, AM355_E_DEVICE, "internal: a head is not among the applied changes");
    stack.push_back(h);
  }
  while (!stack.empty()) {
    const uint32_t i = stack.back();
    stack.pop_back();
    if (seen[i] || !absent(i)) continue;
    seen[i] = 1;
    out.push_back(i);
    for (uint32_t k = g.dep_first[i]; k < g.dep_first[i + 1]; k++) {
      if (g.dep_index[k] >= g.n_staged) return fail(c, AM355_E_DEVICE, "internal: an applied change has a dependency that is not applied");
      stack.push_back(g.dep_index[k]);
    }
  }
  std::reverse(out.begin(), out.end());   // :1994-1996
  return done();
}

// BackendDoc.getMissingDeps(heads), new.js:2014-2028
int missing_deps_impl(am355_ctx* c, const uint8_t* heads, uint32_t n_heads, const uint8_t** hashes, uint32_t* n_out) {
  if (!c || !hashes || !n_out || (n_heads && !heads)) return c ? fail(c, AM355_E_ARG, "null argument") : AM355_E_ARG;
  int rc = served(c, "am355_missing_deps");
  if (rc) return rc;
  (void)hipSetDevice(c->device);
  am355_ctx::GraphIndex& g = c->graph;
  g.out_hashes.clear();
  auto done = [&]() { *hashes = g.out_hashes.data(); *n_out = (uint32_t)(g.out_hashes.size() / 32); return AM355_OK; };
  if (!n_heads && c->pending_change.empty()) return done();
  rc = ensure_index(c);
  if (rc) return rc;
  const uint8_t* hs = c->h_hashes.as<uint8_t>();
  // the candidates: the given heads, the dependencies of the queued changes (read from the staged bytes)
  std::vector<Hash32> all((const Hash32*)heads, (const Hash32*)heads + n_heads);
  std::vector<Hash32> queued;
  for (uint32_t ci : c->pending_change) {
    if (ci >= c->n_changes) return fail(c, AM355_E_DEVICE, "internal: queued change index out of range");
    Hash32 h;
    memcpy(h.b, hs + 32 * (size_t)ci, 32);
    queued.push_back(h);
    const uint64_t offs[2] = {c->raw_off[ci], c->raw_off[ci + 1]};
    ChangeMeta m;
    uint32_t n_entries = 0;
    parse_changes_host(c->raw.data(), offs, 1, &m, &n_entries);
    if (m.flags || (uint64_t)m.deps_off + 32 * (uint64_t)m.n_deps > m.len) return fail(c, AM355_E_DEVICE, "internal: queued change %u does not parse", ci);
    const uint8_t* deps = c->raw.data() + m.base + m.deps_off;
    for (uint32_t k = 0; k < m.n_deps; k++) { memcpy(h.b, deps + 32 * (size_t)k, 32); all.push_back(h); }
  }
  auto less = [](const Hash32& a, const Hash32& b) { return memcmp(a.b, b.b, 32) < 0; };
  std::sort(all.begin(), all.end(), less);   // (a Set, and the result sorted as hex strings: byte order)
  all.erase(std::unique(all.begin(), all.end()), all.end());
  std::sort(queued.begin(), queued.end(), less);
  std::vector<uint32_t> found(all.size());
  rc = lookup(c, all.empty() ? nullptr : all[0].b, (uint32_t)all.size(), found.data());
  if (rc) return rc;
  for (size_t k = 0; k < all.size(); k++)
    if (found[k] == NONE32 && !std::binary_search(queued.begin(), queued.end(), all[k], less)) g.out_hashes.insert(g.out_hashes.end(), all[k].b, all[k].b + 32);
  return done();
}

// am355_test_hash_probe: a table over table_hashes and one probe per query, both on the device, in buffers of the call
int test_hash_probe_impl(am355_ctx* c, const uint8_t* table_hashes, uint32_t n_table, const uint8_t* queries, uint32_t n_queries, uint32_t* out_idx) {
  if (!c || (n_table && !table_hashes) || (n_queries && (!queries || !out_idx))) return c ? fail(c, AM355_E_ARG, "null argument") : AM355_E_ARG;
  if (n_table > MAX_TABLE_CHANGES) return fail(c, AM355_E_UNSUPPORTED, "am355_test_hash_probe: more than 2^30 hashes");
  (void)hipSetDevice(c->device);
  if (!n_queries) return AM355_OK;
  if (!n_table) { std::fill(out_idx, out_idx + n_queries, NONE32); return AM355_OK; }   // (an empty table holds nothing: no launch)
  const uint32_t mask = table_mask_for(n_table);
  DevBuf d_hashes, d_tab, d_q, d_out;
  if (!d_hashes.ensure(32 * (size_t)n_table + 32) || !d_tab.ensure(4 * ((size_t)mask + 1)) || !d_q.ensure(32 * (size_t)n_queries) || !d_out.ensure(4 * (size_t)n_queries))
    return fail(c, AM355_E_NOMEM, "device allocation failed");
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(d_hashes.p, table_hashes, 32 * (size_t)n_table, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(d_tab.p, 0, 4 * ((size_t)mask + 1), st));
  HIPCHK(c, hipMemcpyAsync(d_q.p, queries, 32 * (size_t)n_queries, hipMemcpyHostToDevice, st));
  AM355_LAUNCH_INDEPENDENT(k_graph_insert, dim3(blocks_for(n_table)), dim3(BLOCK), st, (const uint8_t*)d_hashes.as<uint8_t>(), 0u, n_table, d_tab.as<uint32_t>(), mask);
  AM355_LAUNCH_INDEPENDENT(k_hash_probe, dim3(blocks_for(n_queries)), dim3(BLOCK), st, (const uint8_t*)d_hashes.as<uint8_t>(), (const uint32_t*)d_tab.as<uint32_t>(), mask,
                           (const uint8_t*)d_q.as<uint8_t>(), n_queries, d_out.as<uint32_t>());
  HIPCHK(c, hipMemcpyAsync(out_idx, d_out.p, 4 * (size_t)n_queries, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return AM355_OK;
}

extern "C" int am355_find_changes(am355_ctx* c, const uint8_t* hashes, uint32_t n, uint32_t* out_idx) { return guarded(c, [&]() { return find_changes_impl(c, hashes, n, out_idx); }); }
extern "C" int am355_changes_since(am355_ctx* c, const uint8_t* have, uint32_t n_have, const uint32_t** idx, uint32_t* n) { return guarded(c, [&]() { return changes_since_impl(c, have, n_have, idx, n); }); }
extern "C" int am355_changes_added(am355_ctx* c, const uint8_t* other, uint32_t n_other, const uint32_t** idx, uint32_t* n) { return guarded(c, [&]() { return changes_added_impl(c, other, n_other, idx, n); }); }
extern "C" int am355_missing_deps(am355_ctx* c, const uint8_t* heads, uint32_t n_heads, const uint8_t** hashes, uint32_t* n) { return guarded(c, [&]() { return missing_deps_impl(c, heads, n_heads, hashes, n); }); }
extern "C" int am355_test_hash_probe(am355_ctx* c, const uint8_t* table_hashes, uint32_t n_table, const uint8_t* queries, uint32_t n_queries, uint32_t* out_idx) {
  return guarded(c, [&]() { return test_hash_probe_impl(c, table_hashes, n_table, queries, n_queries, out_idx); });
}
extern "C" int am355_set_graph_probe_min(am355_ctx* c, uint32_t n) {
  if (!c) return AM355_E_ARG;
  c->graph_probe_min = n;
  return AM355_OK;
}
extern "C" int am355_graph_query_calls(const am355_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_graph_device;
  out[1] = c->n_graph_host;
  return AM355_OK;
}
