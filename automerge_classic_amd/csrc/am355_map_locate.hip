// Keys of a map resolved to the op ids of their visible values on the device (include/am355.h: am355_map_locate), and the edit by key built
// from them (am355_map_update): what the reference's frontend does in context.setMapKey (frontend/context.js:325-346), deleteMapKey
// (:351-362), deleteTableRow (:531-540) and increment (:546-573) for doc.title = 'x' / delete doc.draft / doc.votes.increment(), without
// a frontend document.
//
// THE RULE (frontend/apply_patch.js:57-79 applyProperties, context.js:576-586 getPred):
//   1. A key holds every visible value under its op id (`props[key][opId]`); the map SHOWS the value of the greatest op id (Lamport order:
//      counter, then actor id).
//   2. The pred of an assignment, a deletion or an increment names the op ids of ALL the key's values.
//   3. An assignment onto a key that shows a Counter throws (context.js:333-335); an increment of a key that shows none throws (:549-551);
//      a deletion of a key without a value makes no op (:355).
//
// ON THE MAP TABLE (include/am355.h am355_ir_map): the records of an object are [map_begin, map_end), one per visible value, sorted by
// (key in UTF-16 code unit order -- a prefix sorts first --, op id). So the values of a key are the run [lb, ub) of records whose key
// equals it, in ascending op id, the shown value is record ub - 1, and both ends are searches. Nothing is taken on trust: the key bytes of
// every record read must lie in the arena, the records on both sides of the run must differ from the key in the right direction, the ids
// inside the run must ascend and no record may carry AM355_MAP_EMPTY -- a miss leaves MF_TABLE and no record of that key is copied.
//
// The object and map tables of a state are current also where in-place merges left its EDIT tables stale (am355_replay.hip: every
// branch of resident_list_verdict / replay_resident that sets ir_stale either leaves ir.obj / ir.map as they were -- a batch of list rows
// only -- or has just rewritten them: resident_map_half, kr_counters, the in-place map merge). So nothing here asks ensure_ir_fresh.
//
// Included at the end of am355_calls.hip, not compiled by itself.
#include "am355_textrec.h"

namespace am355 {

enum MapWord { MW_FLAGS = 0, MW_RECS = 1, MW_WORDS = 2 };
constexpr uint32_t MF_TABLE = 1,   // a record outside the tables, or records that are not in the table's order around the key
                   MF_QUERY = 2,   // key offsets that are out of order or past the blob
                   MF_CAP = 4;     // more records than the result array holds (the same key asked for many times)
constexpr uint32_t MAP_LAST_ROUND = 62;   // a range of up to this many records is the last round's: it looks at them and the two behind
constexpr uint32_t MAP_KEY_LDS = 256;     // a queried key of up to this many bytes is compared from LDS
constexpr uint32_t MAP_FIRST_GATHER = 4096;   // the first gather has room for 2 n + this many records (or the bound of the result, if that is less)

struct MapKeys {
  const am355_ir_map* map;
  uint32_t n_map;
  const uint8_t* arena;
  uint64_t arena_len;
};

// the key of record r against the queried key, in the table's order: < 0 less, 0 equal, > 0 greater. r < n_map.
__device__ __forceinline__ int map_key_order(const MapKeys& t, uint32_t r, const uint8_t* q, uint32_t ql, uint32_t& bad) {
  const uint32_t off = t.map[r].key_off, len = t.map[r].key_len;
  if ((uint64_t)off + len > t.arena_len) { bad |= MF_TABLE; return 0; }
  const uint8_t* p = t.arena + off;
  const uint32_t n = len < ql ? len : ql;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t x = utf16_order_byte(p[k]), y = utf16_order_byte(q[k]);
    if (x != y) return x < y ? -1 : 1;
  }
  return len == ql ? 0 : (len < ql ? -1 : 1);
}
// AM355_MAP_CHILD / AM355_MAP_COUNTER of a record as the frontend sees its value: a counter nobody has incremented carries no total and
// no flag yet, only the type of its `set` (as rec_is_counter of am355_textrec.h has it for a list)
__device__ __forceinline__ uint32_t map_shown_flags(const am355_ir_map& rec) {
  if (rec.flags & AM355_MAP_CHILD) return AM355_MAP_CHILD;
  return (rec.flags & AM355_MAP_COUNTER) || (rec.val_tl & 15u) == 8u ? (uint32_t)AM355_MAP_COUNTER : 0u;
}
__device__ __forceinline__ unsigned long long low_lanes(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// One round after the other of the 64-ary search, by a whole wavefront: [lo, hi) shrinks until it holds at most `limit` records. The
// records in front of lo are `before` the key, those from hi on are not, where before = less (upper == false) or less-or-equal (true).
// Lane k probes pivot lo + (k + 1) * n / 65; the ballot says between which two pivots the boundary lies.
__device__ __forceinline__ void map_narrow(const MapKeys& t, const uint8_t* q, uint32_t ql, bool upper, uint32_t limit, uint32_t lane, uint32_t& lo, uint32_t& hi, uint32_t& bad) {
  while (hi - lo > limit) {
    const uint32_t n = hi - lo;
    const uint32_t pivot = lo + (uint32_t)(((uint64_t)(lane + 1) * n) / 65);   // (< hi: 64 n / 65 < n)
    const int o = map_key_order(t, pivot, q, ql, bad);
    const unsigned long long before = __ballot(upper ? o <= 0 : o < 0);
    const uint32_t c = (uint32_t)__popcll(before);
    if (before != low_lanes(c)) bad |= MF_TABLE;   // (the pivots are not in order)
    const uint32_t nlo = c ? lo + (uint32_t)(((uint64_t)c * n) / 65) + 1 : lo, nhi = c < 64 ? lo + (uint32_t)(((uint64_t)(c + 1) * n) / 65) : hi;
    lo = nlo;
    hi = nhi < nlo ? nlo : nhi;   // (strictly fewer records than before: every round ends)
  }
}

// What both locate kernels leave for key i: the run's first record, its length (0 where a check missed) and the flags of the shown value.
// lane / stride: the threads that share the walk over the run (a wavefront, or one thread).
__device__ __forceinline__ uint32_t map_check_run(const MapKeys& t, const uint8_t* q, uint32_t ql, uint32_t begin, uint32_t end, uint32_t lb, uint32_t ub, uint32_t lane, uint32_t stride) {
  uint32_t bad = 0;
  if (lane == 0 && lb > begin && map_key_order(t, lb - 1, q, ql, bad) >= 0) bad |= MF_TABLE;
  if (lane == stride - 1 && ub < end && map_key_order(t, ub, q, ql, bad) <= 0) bad |= MF_TABLE;
  for (uint32_t r = lb + lane; r < ub; r += stride) {
    const am355_ir_map& rec = t.map[r];
    if ((rec.flags & AM355_MAP_EMPTY) || map_key_order(t, r, q, ql, bad) != 0) bad |= MF_TABLE;
    if (r + 1 < ub) {
      const am355_ir_map& nx = t.map[r + 1];
      if (!(rec.id_ctr < nx.id_ctr || (rec.id_ctr == nx.id_ctr && rec.id_actor < nx.id_actor))) bad |= MF_TABLE;
    }
  }
  return bad;
}

// The queries of both kernels: key i = kbytes[koff[i], koff[i + 1]), in pinned host memory or in device memory.
struct MapQuery {
  const uint8_t* kbytes;
  const uint32_t* koff;
  uint32_t kbytes_len, n;
  const am355_ir_object* obj;   // the device's object table when the host does not know the object's range (else null) ...
  uint32_t oi, begin, end;      // ... the object's index | its range of records as the host knows it
};
__device__ __forceinline__ bool map_query_key(const MapQuery& m, uint32_t i, uint32_t& ko, uint32_t& kl) {
  const uint32_t a = m.koff[i], b = m.koff[i + 1];
  ko = kl = 0;
  if (a > b || b > m.kbytes_len) return false;
  ko = a; kl = b - a;
  return true;
}
__device__ __forceinline__ bool map_query_range(const MapKeys& t, const MapQuery& m, uint32_t& begin, uint32_t& end) {
  begin = m.begin; end = m.end;
  if (m.obj) { begin = m.obj[m.oi].map_begin; end = m.obj[m.oi].map_end; }
  if (begin <= end && end <= t.n_map) return true;
  begin = end = 0;
  return false;
}

// Locate, one WAVEFRONT per key. The key goes to LDS first (one read of it, however many rounds follow). Lower bound: narrowing rounds
// down to MAP_LAST_ROUND records, then the last round over them and the two records behind (the invariant says nothing about record
// hi, and a run of one that begins there ends at hi + 1): lanes that are less, lanes that are equal. Only a run that reaches the end of
// that window is followed further: by a second 64-ary search, for the first greater key, over what lies behind the window.
__global__ __launch_bounds__(BLOCK) void kmap_locate(MapKeys t, MapQuery m, uint32_t* __restrict__ words, uint32_t* __restrict__ lb_out, uint32_t* __restrict__ num_out,
                                                     uint32_t* __restrict__ kflags_out) {
  __shared__ uint8_t s_key[BLOCK / WAVE][MAP_KEY_LDS];
  const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE, i = blockIdx.x * (BLOCK / WAVE) + w;
  const bool live = i < m.n;
  uint32_t bad = 0, ko = 0, kl = 0;
  if (live && !map_query_key(m, i, ko, kl)) bad |= MF_QUERY;
  if (live && kl <= MAP_KEY_LDS)
    for (uint32_t k = lane; k < kl; k += WAVE) s_key[w][k] = m.kbytes[ko + k];
  __syncthreads();   // (only a wavefront's own writes need ordering: the barrier of the workgroup is the plain way to say it, and every thread is still here)
  if (!live) return;   // (a whole wavefront: i is the wavefront's)
  const uint8_t* q = kl <= MAP_KEY_LDS ? s_key[w] : m.kbytes + ko;
  uint32_t begin, end;
  if (!map_query_range(t, m, begin, end)) bad |= MF_TABLE;
  uint32_t lo = begin, hi = end;
  map_narrow(t, q, kl, false, MAP_LAST_ROUND, lane, lo, hi, bad);
  const uint32_t wend = end - hi < 2 ? end : hi + 2;   // (at most 64 records)
  const uint32_t r = lo + lane;
  const bool in = r < wend;
  const int o = in ? map_key_order(t, r, q, kl, bad) : 1;
  const unsigned long long less = __ballot(in && o < 0), equal = __ballot(in && o == 0);
  const uint32_t nl = (uint32_t)__popcll(less), ne = (uint32_t)__popcll(equal);
  if (less != low_lanes(nl) || (ne && equal != (low_lanes(ne) << nl))) bad |= MF_TABLE;
  const uint32_t lb = lo + nl;
  uint32_t ub = lb + ne;
  if (ub == wend && wend < end) {   // the run may go on behind the window
    uint32_t lo2 = wend, hi2 = end;
    map_narrow(t, q, kl, true, WAVE, lane, lo2, hi2, bad);
    const uint32_t r2 = lo2 + lane;
    const bool in2 = r2 < hi2;
    const int o2 = in2 ? map_key_order(t, r2, q, kl, bad) : 1;
    const unsigned long long le = __ballot(in2 && o2 <= 0);
    const uint32_t nle = (uint32_t)__popcll(le);
    if (le != low_lanes(nle)) bad |= MF_TABLE;
    ub = lo2 + nle;
  }
  if (ub < lb || ub > end) { bad |= MF_TABLE; ub = lb; }
  if (!(bad & MF_TABLE)) bad |= map_check_run(t, q, kl, begin, end, lb, ub, lane, WAVE);
  const uint32_t f = (__ballot((bad & MF_TABLE) != 0) ? MF_TABLE : 0u) | (__ballot((bad & MF_QUERY) != 0) ? MF_QUERY : 0u);
  if (lane) return;
  if (f) atomicOr(&words[MW_FLAGS], f);
  const uint32_t num = f ? 0u : ub - lb;
  lb_out[i] = lb;
  num_out[i] = num;
  kflags_out[i] = num ? map_shown_flags(t.map[ub - 1]) : 0u;
}

// The same answer by one THREAD per key: two binary searches. (am355_set_map_locate_thread: the measurement of the two against each
// other, profiles/map_update_timings.txt.)
__global__ __launch_bounds__(BLOCK) void kmap_locate_thread(MapKeys t, MapQuery m, uint32_t* __restrict__ words, uint32_t* __restrict__ lb_out, uint32_t* __restrict__ num_out,
                                                            uint32_t* __restrict__ kflags_out) {
  const uint32_t i = gtid();
  if (i >= m.n) return;
  uint32_t bad = 0, ko, kl, begin, end;
  if (!map_query_key(m, i, ko, kl)) bad |= MF_QUERY;
  if (!map_query_range(t, m, begin, end)) bad |= MF_TABLE;
  const uint8_t* q = m.kbytes + ko;
  uint32_t a = begin, b = end;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (map_key_order(t, mid, q, kl, bad) < 0) a = mid + 1; else b = mid;
  }
  const uint32_t lb = a;
  b = end;
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (map_key_order(t, mid, q, kl, bad) <= 0) a = mid + 1; else b = mid;
  }
  const uint32_t ub = a;
  if (!(bad & MF_TABLE)) bad |= map_check_run(t, q, kl, begin, end, lb, ub, 0, 1);
  if (bad) atomicOr(&words[MW_FLAGS], bad);
  const uint32_t num = bad ? 0u : ub - lb;
  lb_out[i] = lb;
  num_out[i] = num;
  kflags_out[i] = num ? map_shown_flags(t.map[ub - 1]) : 0u;
}

// Gather, one thread per key: its hit -- where its records stand in the result, how many, the flags of the shown value -- and the records
// of its run as they are. Hit i and record p go where pinned_or_spill says; a run that would pass `cap` is not copied and leaves MF_CAP.
__global__ __launch_bounds__(BLOCK) void kmap_gather(const am355_ir_map* __restrict__ map, const uint32_t* __restrict__ lb, const uint32_t* __restrict__ num,
                                                     const uint32_t* __restrict__ kflags, const uint32_t* __restrict__ first, uint32_t n, uint32_t cap, uint32_t* __restrict__ words,
                                                     am355_map_hit* __restrict__ hit_pinned, am355_map_hit* __restrict__ hit_spill, am355_ir_map* __restrict__ rec_pinned,
                                                     am355_ir_map* __restrict__ rec_spill) {
  const uint32_t i = gtid();
  if (i >= n) return;
  const uint32_t f = first[i];
  uint32_t cnt = num[i];
  if ((uint64_t)f + cnt > cap) { atomicOr(&words[MW_FLAGS], (uint32_t)MF_CAP); cnt = 0; }
  am355_map_hit* h = pinned_or_spill(hit_pinned, hit_spill, i);
  h->first = f; h->num = cnt; h->flags = kflags[i]; h->pad = 0;
  for (uint32_t k = 0; k < cnt; k++) *pinned_or_spill(rec_pinned, rec_spill, f + k) = map[lb[i] + k];
}

}  // namespace am355

namespace {

struct MapLocated {
  const am355_map_hit* hits = nullptr;
  const am355_ir_map* recs = nullptr;
  uint32_t n_recs = 0, type = 0, index = 0;
};

// What both calls share: the hits of the n keys (key i = keys[key_off[i], key_off[i + 1])) in the map or table (obj_ctr, obj_actor) and
// the records of their runs.
int map_locate_core(am355_ctx* c, const char* who, uint32_t open_flags, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const uint8_t* keys,
                    const uint32_t* key_off, uint32_t n, MapLocated& out) {
  { int src = call_open_state(c, who, open_flags); if (src) return src; }
  out = MapLocated();
  for (uint32_t k = 0; k < n; k++)
    if (key_off[k + 1] < key_off[k]) return fail(c, AM355_E_ARG, "%s: key offsets out of order", who);
  hipStream_t st = c->stream;
  const uint32_t NO = c->counts.n_objects, NM = c->counts.n_map_emit;
  // ---- the object: _root is index 0 of the table and a map; any other is looked up as for the calls on a Text ----
  bool range_known = false;
  uint32_t oi = 0, type = 0, begin = 0, end = 0;
  if (obj_ctr == 0 && actor_len == 0) {
    if (!NO) return fail(c, AM355_E_DEVICE, "internal: a state without an object table");
    if (NM == 0) range_known = true;
    else if (c->h_tables_current && c->hir.objects && c->hir.n_objects == NO) { begin = c->hir.objects[0].map_begin; end = c->hir.objects[0].map_end; range_known = true; }
  } else {
    FoundObject f;
    { int lrc = object_lookup(c, obj_ctr, obj_actor, actor_len, true, &c->n_map_launches, f); if (lrc) return lrc; }
    oi = f.index; type = f.type; begin = f.begin; end = f.end;
    range_known = true;
  }
  if (type != 0 && type != 6) return fail(c, AM355_E_ARG, "not a map object");
  if (range_known && (begin > end || end > NM)) return fail(c, AM355_E_DEVICE, "internal: map range [%u, %u) of object %u outside the %u records", begin, end, oi, NM);
  out.type = type; out.index = oi;
  if (!c->h_mloc_hits.ensure(((size_t)(n ? n : 1)) * sizeof(am355_map_hit)) || !c->h_mloc_recs.ensure(sizeof(am355_ir_map)))
    return fail(c, AM355_E_NOMEM, "host allocation failed (map locate)");
  out.hits = c->h_mloc_hits.as<am355_map_hit>();
  out.recs = c->h_mloc_recs.as<am355_ir_map>();
  if (n == 0) return AM355_OK;   // nothing asked: nothing to launch
  if (range_known && begin == end) {   // an object without records: every key is absent, nothing to launch
    memset(c->h_mloc_hits.p, 0, (size_t)n * sizeof(am355_map_hit));
    return AM355_OK;
  }
  if (!c->mb.arena) return fail(c, AM355_E_DEVICE, "internal: the arena of the state is not on the device");
  // The bound of the result: every record of the object once, and one more per key for keys that are asked for again. The arrays are
  // NOT sized for it (one key asked of a map of a million records would pin 40 MB): the first gather has room for two records a key and
  // 4,096 more, which holds every call but one whose keys carry many conflicting values; that one learns the count from the scan in its
  // one wait and gathers a second time into arrays of that size.
  const uint32_t R = range_known ? end - begin : NM;
  const uint64_t full64 = (uint64_t)R + n;
  if (full64 > 0xffffffffull) return fail(c, AM355_E_UNSUPPORTED, "%s: more than 2^32 records possible", who);
  const uint32_t full = (uint32_t)full64, kbytes = key_off[n] - key_off[0];
  uint32_t cap = (uint32_t)std::min<uint64_t>(full, 2 * (uint64_t)n + MAP_FIRST_GATHER);
  // more keys than are read from pinned memory, or a key that is compared where it lies (every probe of it would cross the link): one copy up
  bool up = n > LOCATE_PINNED_RUNS;
  for (uint32_t k = 0; k < n && !up; k++) up = key_off[k + 1] - key_off[k] > MAP_KEY_LDS;
  // words | lb, num, kflags, first | the keys (offsets, then bytes) when they go up | scan workspace
  const size_t b_words = carve_size(MW_WORDS, 4), b_arr = carve_size(n, 4), b_koff = carve_size((size_t)n + 1, 4), b_keys = up ? b_koff + carve_round(kbytes) : 0,
               b_ws = carve_round(scan_workspace_bytes(n));
  const uint32_t spill_hits = n > LOCATE_PINNED_RUNS ? n - LOCATE_PINNED_RUNS : 0u;
  auto room_for = [&](uint32_t records) {   // the pinned array and the spill behind it for that many records
    const uint32_t spill = records > LOCATE_PINNED_RUNS ? records - LOCATE_PINNED_RUNS : 0u;
    return (!spill || c->d_mloc_recs.ensure((size_t)spill * sizeof(am355_ir_map))) && c->h_mloc_recs.ensure((size_t)(records ? records : 1) * sizeof(am355_ir_map));
  };
  if (!c->d_mloc.ensure(b_words + 4 * b_arr + b_keys + b_ws) || (spill_hits && !c->d_mloc_hits.ensure((size_t)spill_hits * sizeof(am355_map_hit))) || !room_for(cap) ||
      !c->h_mloc_keys.ensure(b_koff + kbytes + 1) || !c->text_sig.ready())
    return fail(c, AM355_E_NOMEM, "allocation failed (map locate)");
  out.recs = c->h_mloc_recs.as<am355_ir_map>();
  uint8_t* dp = c->d_mloc.as<uint8_t>();
  uint32_t* dw = (uint32_t*)dp;
  uint32_t* arr = (uint32_t*)(dp + b_words);
  const size_t step = b_arr / 4;
  uint32_t *d_lb = arr, *d_num = arr + step, *d_kf = arr + 2 * step, *d_first = arr + 3 * step;
  uint8_t* d_keys = dp + b_words + 4 * b_arr;
  void* d_ws = dp + b_words + 4 * b_arr + b_keys;
  // the queries in pinned memory, offsets from 0: read there by the kernel, or copied up in one piece
  uint32_t* h_koff = c->h_mloc_keys.as<uint32_t>();
  uint8_t* h_kbytes = c->h_mloc_keys.as<uint8_t>() + b_koff;
  for (uint32_t k = 0; k <= n; k++) h_koff[k] = key_off[k] - key_off[0];
  if (kbytes) memcpy(h_kbytes, keys + key_off[0], kbytes);
  MapQuery m{h_kbytes, h_koff, kbytes, n, range_known ? nullptr : (const am355_ir_object*)c->ir.obj, oi, begin, end};
  if (up) {
    HIPCHK(c, hipMemcpyAsync(d_keys, c->h_mloc_keys.p, b_koff + kbytes, hipMemcpyHostToDevice, st));
    m.koff = (const uint32_t*)d_keys;
    m.kbytes = d_keys + b_koff;
  }
  const MapKeys t{(const am355_ir_map*)c->ir.map, NM, (const uint8_t*)c->mb.arena, (uint64_t)c->raw.size()};
  HIPCHK(c, hipMemsetAsync(dw, 0, MW_WORDS * 4, st));
  if (c->map_locate_thread) AM355_LAUNCH_INDEPENDENT(kmap_locate_thread, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), st, t, m, dw, d_lb, d_num, d_kf);
  else hipLaunchKernelGGL(kmap_locate, dim3((n + BLOCK / WAVE - 1) / (BLOCK / WAVE)), dim3(BLOCK), 0, st, t, m, dw, d_lb, d_num, d_kf);
  exclusive_scan_u32(d_num, d_first, n, dw + MW_RECS, d_ws, st);
  auto gather = [&]() {
    AM355_LAUNCH_INDEPENDENT(kmap_gather, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), st, t.map, (const uint32_t*)d_lb, (const uint32_t*)d_num, (const uint32_t*)d_kf,
                             (const uint32_t*)d_first, n, cap, dw, c->h_mloc_hits.as<am355_map_hit>(), c->d_mloc_hits.as<am355_map_hit>(), c->h_mloc_recs.as<am355_ir_map>(),
                             c->d_mloc_recs.as<am355_ir_map>());
  };
  gather();
  c->n_map_launches += 4;
  // the one wait of the call: flag word, number of records
  HIPCHK(c, c->text_sig.fetch(dw, MW_WORDS, 0, st));
  const uint32_t* hw = c->text_sig.words();
  uint32_t mf = hw[MW_FLAGS];
  const uint32_t nr = hw[MW_RECS];
  if (mf == MF_CAP && nr > cap && nr <= full) {   // more records than the first gather had room for: the searches and the scan stand, the gather runs again
    cap = nr;
    if (!room_for(cap)) return fail(c, AM355_E_NOMEM, "allocation failed (map locate)");
    HIPCHK(c, hipMemsetAsync(dw + MW_FLAGS, 0, 4, st));
    gather();
    c->n_map_launches += 2;
    HIPCHK(c, c->text_sig.fetch(dw, 1, 0, st));
    mf = c->text_sig.words()[MW_FLAGS];
  }
  out.recs = c->h_mloc_recs.as<am355_ir_map>();
  if (mf & MF_QUERY) return fail(c, AM355_E_DEVICE, "internal: the key offsets of the query did not arrive as they were sent");
  if (mf & MF_TABLE) return fail(c, AM355_E_DEVICE, "internal: the map records of object %u are not in the table's order, or lie outside the tables", oi);
  if ((mf & MF_CAP) || nr > cap) return fail(c, AM355_E_ARG, "%s: the same keys asked for so often that more than %u records would be returned: ask for a key once", who, full);
  { int src = spill_down(c, c->h_mloc_hits.as<am355_map_hit>(), (const am355_map_hit*)c->d_mloc_hits.as<am355_map_hit>(), n); if (src) return src; }
  { int src = spill_down(c, c->h_mloc_recs.as<am355_ir_map>(), (const am355_ir_map*)c->d_mloc_recs.as<am355_ir_map>(), nr); if (src) return src; }
  // every index the host follows is checked before it is used
  for (uint32_t k = 0; k < n; k++)
    if ((uint64_t)out.hits[k].first + out.hits[k].num > nr) return fail(c, AM355_E_DEVICE, "internal: hit %u names records outside the %u gathered", k, nr);
  out.n_recs = nr;
  return AM355_OK;
}

int map_locate_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const uint8_t* keys, const uint32_t* key_off, uint32_t n,
                    const am355_map_hit** hits, const am355_ir_map** recs, uint32_t* n_recs) {
  if (!c) return AM355_E_ARG;
  if (!hits || !recs || !n_recs || (!obj_actor && actor_len) || (n && (!key_off || (!keys && key_off[n] != key_off[0])))) return fail(c, AM355_E_ARG, "am355_map_locate: null argument");
  MapLocated l;
  const int rc = map_locate_core(c, "am355_map_locate", 0, obj_ctr, obj_actor, actor_len, keys, key_off, n, l);
  *hits = l.hits; *recs = l.recs; *n_recs = l.n_recs;
  return rc;
}

int map_update_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const am355_map_op* ops, uint32_t n_ops, const uint8_t* strings,
                    uint32_t strings_len, const am355_local_value* values, uint32_t n_values, const uint8_t* author, size_t author_len, int64_t time, const uint8_t* message,
                    uint32_t message_len, const uint8_t** change, size_t* len) {
  if (!c) return AM355_E_ARG;
  auto refused = [&](int code) { c->n_map_refused++; return code; };
  if (!change || !len || (!obj_actor && actor_len) || !author || !author_len || (n_ops && !ops) || (n_values && !values) || (!strings && strings_len) || (!message && message_len))
    return refused(fail(c, AM355_E_ARG, "am355_map_update: null argument"));
  if (!list_values_ok(values, n_values, strings_len)) return refused(fail(c, AM355_E_ARG, "am355_map_update: a string value outside `strings`"));
  const TraceLap lap("map_update:", 26);
  *change = nullptr; *len = 0;
  // ---- the ops by themselves: kinds, key ranges, value indexes; a key named twice ----
  std::vector<uint32_t> key_off(1, 0);
  std::vector<uint8_t> keys;
  std::vector<std::string> seen;
  for (uint32_t k = 0; k < n_ops; k++) {
    const am355_map_op& op = ops[k];
    if (op.kind != AM355_MOP_SET && op.kind != AM355_MOP_DELETE && op.kind != AM355_MOP_INC) return refused(fail(c, AM355_E_ARG, "am355_map_update: op %u of unknown kind %u", k, op.kind));
    if ((uint64_t)op.key_off + op.key_len > strings_len) return refused(fail(c, AM355_E_ARG, "am355_map_update: a key outside `strings`"));
    if (op.kind == AM355_MOP_SET && op.value >= n_values) return refused(fail(c, AM355_E_ARG, "am355_map_update: op %u names value %u of %u", k, op.value, n_values));
    keys.insert(keys.end(), strings + op.key_off, strings + op.key_off + op.key_len);
    key_off.push_back((uint32_t)keys.size());
    seen.emplace_back((const char*)strings + op.key_off, op.key_len);
  }
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
    return refused(fail(c, AM355_E_ARG, "am355_map_update: a key named twice in one call (the second op's pred would be the first op: not built)"));
  // ---- every key located in one query, on the state of the document's rebuilt changes, whose clock, heads and max_op the request needs.
  // A context without a state is Backend.init(): _root alone, without a key -- nothing to search ----
  MapLocated l;
  int rc;
  const bool onto_nothing = !c->staged;
  std::vector<am355_map_hit> none(onto_nothing ? (size_t)n_ops + 1 : 0, am355_map_hit{0, 0, 0, 0});
  if (onto_nothing) {
    if (c->shard_world > 1) return refused(fail(c, AM355_E_UNSUPPORTED, "am355_map_update on a sharded context"));
    if (obj_ctr || actor_len) return refused(fail(c, AM355_E_ARG, "no such object: an empty document holds _root alone"));
    l.hits = none.data();
  } else {
    rc = map_locate_core(c, "am355_map_update", TO_CHANGE_STATE | TO_NO_QUEUE, obj_ctr, obj_actor, actor_len, keys.data(), key_off.data(), n_ops, l);
    if (rc) return refused(rc);
  }
  lap("located");
  // ---- the request, op by op as the frontend would meet them: its first exception is the call's ----
  const uint32_t NA = (uint32_t)c->actors.size();
  const std::string me((const char*)author, author_len), obj_a = actor_len ? std::string((const char*)obj_actor, actor_len) : std::string();
  std::vector<std::string> others;   // (_root has no actor)
  if (actor_len) others.push_back(obj_a);
  std::vector<am355_local_op> flat;
  std::vector<std::pair<uint32_t, uint32_t>> rank_preds;   // (actor rank, counter) until the change's actor table is known
  std::vector<am355_local_value> vals;
  for (uint32_t k = 0; k < n_ops; k++) {
    const am355_map_op& op = ops[k];
    const am355_map_hit& h = l.hits[k];
    const bool counter = h.num && (h.flags & AM355_MAP_COUNTER);
    if (l.type == 6 && (op.kind != AM355_MOP_DELETE || h.num > 1))   // (a table row is set through Table.add, which makes an object: context.js:505-526)
      return refused(fail(c, AM355_E_UNSUPPORTED, "am355_map_update: on a table object only the deletion of a row is served: JS path"));
    if (op.kind == AM355_MOP_SET) {
      if (!op.key_len) return refused(fail(c, AM355_E_ARG, "The key of a map entry must not be an empty string"));   // context.js:293-295
      if (counter) return refused(fail(c, AM355_E_INVALID, "Cannot overwrite a Counter object; use .increment() or .decrement() to change its value."));   // :333-335
    } else if (op.kind == AM355_MOP_INC) {
      if (!counter) return refused(fail(c, AM355_E_INVALID, "Only counter values can be incremented"));   // :549-551
    } else if (!h.num) continue;   // a deletion of a key without a value: no op (:355)
    am355_local_op o{};
    o.action = op.kind == AM355_MOP_SET ? 1u : op.kind == AM355_MOP_DELETE ? 3u : 5u;
    o.obj_ctr = (uint32_t)obj_ctr;
    o.key_kind = AM355_LK_STRING;
    o.key_off = op.key_off; o.key_len = op.key_len;
    o.multi = 1;
    o.val_first = (uint32_t)vals.size();
    if (op.kind == AM355_MOP_SET) vals.push_back(values[op.value]);
    if (op.kind == AM355_MOP_INC) vals.push_back(am355_local_value{AM355_LV_INT, 0, 0, 0, (uint64_t)op.delta});
    o.pred_first = (uint32_t)rank_preds.size(); o.pred_num = h.num;
    for (uint32_t q = 0; q < h.num; q++) {
      const am355_ir_map& rec = l.recs[h.first + q];
      if (rec.id_actor >= NA) return refused(fail(c, AM355_E_DEVICE, "internal: a map record names an actor outside the table"));
      rank_preds.emplace_back(rec.id_actor, rec.id_ctr);
      others.push_back(c->actors[rec.id_actor]);
    }
    flat.push_back(o);
  }
  if (flat.empty()) { c->n_map_served++; return AM355_OK; }   // (nothing but deletions of absent keys: no change, as a splice that changes nothing)
  if ((onto_nothing ? 0 : c->max_op) + flat.size() > 0xffffffffull) return refused(fail(c, AM355_E_UNSUPPORTED, "counters beyond 2^32"));
  const SpliceActors act(me, others);
  const uint32_t obj_local = actor_len ? act.local(obj_a) : NONE32;
  std::vector<am355_local_pred> preds;
  for (am355_local_op& o : flat) o.obj_actor = obj_local;
  for (const auto& p : rank_preds) preds.push_back(am355_local_pred{act.local(c->actors[p.first]), p.second});
  lap("request built");
  rc = splice_apply(c, act, author, author_len, time, message, message_len, strings, strings_len, flat, vals, preds, change, len, onto_nothing);
  lap("applied");
  if (rc) return refused(rc);
  c->n_map_served++;
  return AM355_OK;
}

}  // namespace

extern "C" int am355_map_locate(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const uint8_t* keys, const uint32_t* key_off, uint32_t n,
                                const am355_map_hit** hits, const am355_ir_map** recs, uint32_t* n_recs) {
  return guarded(c, [&]() { return map_locate_impl(c, obj_ctr, obj_actor, actor_len, keys, key_off, n, hits, recs, n_recs); });
}
extern "C" int am355_map_update(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const am355_map_op* ops, uint32_t n_ops, const uint8_t* strings,
                                uint32_t strings_len, const am355_local_value* values, uint32_t n_values, const uint8_t* author, size_t author_len, int64_t time,
                                const uint8_t* message, uint32_t message_len, const uint8_t** change, size_t* len) {
  return guarded(c, [&]() {
    return map_update_impl(c, obj_ctr, obj_actor, actor_len, ops, n_ops, strings, strings_len, values, n_values, author, author_len, time, message, message_len, change, len);
  });
}
extern "C" int am355_map_calls(const am355_ctx* c, uint64_t out[3]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_map_served;
  out[1] = c->n_map_refused;
  out[2] = c->n_map_launches;
  return AM355_OK;
}
extern "C" int am355_set_map_locate_thread(am355_ctx* c, int on) {
  if (!c) return AM355_E_ARG;
  c->map_locate_thread = on != 0;
  return AM355_OK;
}
extern "C" int am355_map_locate_limits(uint32_t out[4]) {
  if (!out) return AM355_E_ARG;
  out[0] = MAP_LAST_ROUND; out[1] = LOCATE_PINNED_RUNS; out[2] = LOCATE_PINNED_RUNS; out[3] = MAP_FIRST_GATHER;
  return AM355_OK;
}
