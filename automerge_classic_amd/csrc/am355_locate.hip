// Positions of a Text resolved to ids on the device (include/am355.h: am355_text_locate), and the positional edit built from them
// (am355_text_splice): what the reference's frontend does in context.splice (frontend/context.js:441-502) for text.deleteAt /
// text.insertAt, without a frontend document. A caller that keeps a Text on the engine names what it edits by position; a change
// request names list elements by elemId and, for a deletion, by the op id of the value that goes (`pred`). Both are read here from the
// whole-document edit records in HBM, compressed into the runs context.splice would merge into `multiOp` deletions, and only the runs
// cross the link: a 100,000-character deletion inside pasted text is one run of 24 bytes.
//
// THE RULE (frontend/context.js:452-496 splice, :576-586 getPred, frontend/apply_patch.js:231-255 updateTextObject):
//   1. An element of a Text has an elemId and exactly one pred: an `insert` edit gives pred = [edit.opId], a `multi-insert` edit gives
//      element i elemId = edit.elemId + i and pred = [that elemId], an `update` edit REPLACES the element with pred = [edit.opId] and the
//      elemId kept (apply_patch.js:232-250). So the pred is the op id of the last edit of the element's index.
//   2. A deletion joins the one before it as multiOp iff the elemId actors are equal and the elemId counters consecutive, and the pred
//      actors are equal and the pred counters consecutive (context.js:483-486; "both have exactly one pred" always holds by 1).
//   3. An element that is a Counter cannot be deleted (context.js:455-471).
//
// ON THE RECORD TABLE (am355_textrec.h, which proves it, (a) - (h)): for element j let hi be the LAST record with hi.index <= j. Then
//     elemId = (hi.elem_ctr + (j - hi.index), hi.elem_actor)        pred = (hi.id_ctr + (j - hi.index), hi.id_actor)
// and the element is a counter iff hi is one (rec_is_counter). kl_check verifies the premises per record before anything is searched
// (rec_premises); its last thread leaves the object's length.
//
// Included at the end of am355_calls.hip, not compiled by itself.
#include "am355_textrec.h"

namespace am355 {

// device words of a call (d_loc)
enum LocWord { LW_FLAGS = 0, LW_LENGTH = 1, LW_RUNS = 2, LW_COUNTERS = 3, LW_WORDS = 4 };
constexpr uint32_t LF_RANGE = RF_CALL;   // flag bit of a call: the queried range reaches past the object's length

// Check pass, one thread per record of the object: the premises of the searches. The last record's thread leaves the length.
__global__ __launch_bounds__(BLOCK) void kl_check(TextRecs t, uint32_t* __restrict__ words) {
  const uint32_t k = gtid();
  if (k >= t.R) return;
  uint32_t count, length;
  const uint32_t err = rec_premises(t, k, count, length);
  if (err) atomicOr(&words[LW_FLAGS], err);
  else if (k + 1 == t.R) words[LW_LENGTH] = length;
}
void launch_text_check(const TextRecs& t, uint32_t* words, hipStream_t st) {
  AM355_LAUNCH_INDEPENDENT(kl_check, dim3((t.R + BLOCK - 1) / BLOCK), dim3(BLOCK), st, t, words);
}

// Locate, one thread per queried element first + i: ids[i], counter[i] and head[i] = 1 iff the element does not continue the one before
// it by the multiOp rule. Element 0 is a head, and so is element `lead` (1: the range begins one element early -- the reference element
// of an insertion, which is no deletion and must not merge with the first one; 0: no such element). The neighbour's ids come from LDS;
// the first thread of a workgroup searches for them again.
__global__ __launch_bounds__(BLOCK) void kl_locate(TextRecs t, uint32_t first, uint32_t n, uint32_t lead, uint32_t* __restrict__ words, uint4* __restrict__ ids,
                                                   uint32_t* __restrict__ head, uint32_t* __restrict__ counter) {
  __shared__ uint4 s_ids[BLOCK];
  const uint32_t i = gtid();
  const uint32_t length = words[LW_LENGTH];   // (kl_check, the launch before; 0 when it found the table broken)
  const bool live = i < n && (uint64_t)first + i < length;
  uint4 me = uint4{0, 0, 0, 0};
  uint32_t cnt = 0;
  if (live) me = locate_ids(t, first + i, cnt);
  s_ids[threadIdx.x] = me;
  __syncthreads();
  if (i >= n) return;
  if (!live) {
    atomicOr(&words[LW_FLAGS], (uint32_t)LF_RANGE);
    ids[i] = me; head[i] = 0; counter[i] = 0;
    return;
  }
  uint32_t h = 1;
  if (i != 0 && i != lead) {
    uint32_t pc;
    const uint4 p = threadIdx.x ? s_ids[threadIdx.x - 1] : locate_ids(t, first + i - 1, pc);
    if (p.y == me.y && p.x + 1 == me.x && p.w == me.w && p.z + 1 == me.z) h = 0;
  }
  ids[i] = me; head[i] = h; counter[i] = cnt;
  if (cnt) atomicAdd(&words[LW_COUNTERS], 1u);   // (counters inside a Text are rare: no contention to speak of)
}

// Compaction, one thread per queried element: a head writes its run -- ids, the distance to the next head (found by binary search over
// the scanned head bits: pos[x] = heads in front of x, non-decreasing), whether a counter is among its elements (only when the range
// holds a counter at all does the head walk its run's counter bits). Run r goes where pinned_or_spill says.
__global__ __launch_bounds__(BLOCK) void kl_runs(const uint4* __restrict__ ids, const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos,
                                                 const uint32_t* __restrict__ counter, uint32_t n, const uint32_t* __restrict__ words, am355_text_run* __restrict__ pinned,
                                                 am355_text_run* __restrict__ spill) {
  const uint32_t i = gtid();
  if (i >= n || !head[i]) return;
  const uint32_t r = pos[i];
  uint32_t lo = i, hi = n;   // pos[lo] <= r + 1 < pos[hi]: everything up to and including the next head has at most r + 1 heads in front
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (pos[mid] <= r + 1) lo = mid; else hi = mid;
  }
  const uint32_t end = (lo > i && head[lo]) ? lo : lo + 1;   // the next head, or n
  uint32_t counters = 0;
  if (words[LW_COUNTERS])
    for (uint32_t x = i; x < end; x++) counters |= counter[x];
  const uint4 me = ids[i];
  am355_text_run* out = pinned_or_spill(pinned, spill, r);
  out->elem_ctr = me.x; out->elem_actor = me.y; out->pred_ctr = me.z; out->pred_actor = me.w;
  out->count = end - i;
  out->flags = counters ? AM355_RUN_COUNTER : 0u;
}

}  // namespace am355

namespace {

// What both calls share: the runs of [first, first + n) of the object, *length, and *past = 1 when the range reaches past it (no runs
// then). lead: see kl_locate. who, open_flags: the call and what its opening asks for (text_open).
int locate_core(am355_ctx* c, const char* who, uint32_t open_flags, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t first, uint64_t n, uint32_t lead,
                const am355_text_run** runs, uint32_t* n_runs, uint64_t* length, bool* past) {
  TextObject o;
  { int orc = text_open(c, who, obj_ctr, obj_actor, actor_len, open_flags, &c->n_locate_launches, o); if (orc) return orc; }
  hipStream_t st = c->stream;
  const uint32_t R = o.recs.R, oi = o.index;
  *runs = nullptr; *n_runs = 0; *length = 0; *past = false;
  if (!c->h_loc_runs.ensure(sizeof(am355_text_run))) return fail(c, AM355_E_NOMEM, "host allocation failed (locate)");
  *runs = c->h_loc_runs.as<am355_text_run>();
  if (R == 0) {   // an empty Text: nothing to launch
    *past = first + n > 0 || first + n < first;
    return AM355_OK;
  }
  // (a range the 32-bit positions cannot hold lies past every Text; the length is still wanted)
  const bool fits = first <= 0xffffffffull && n <= 0xffffffffull && first + n <= 0xffffffffull;
  const uint32_t N = fits ? (uint32_t)n : 0u, F = fits ? (uint32_t)first : 0u;
  const size_t b_words = carve_size(LW_WORDS, 4), b_ids = carve_size(N, 16), b_arr = carve_size(N, 4), b_ws = carve_round(scan_workspace_bytes(N ? N : 1));   // ids | head, counter, pos | scan workspace
  const uint32_t spill_max = N > LOCATE_PINNED_RUNS ? N - LOCATE_PINNED_RUNS : 0u;
  if (!c->d_loc.ensure(b_words + b_ids + 3 * b_arr + b_ws) || (spill_max && !c->d_loc_runs.ensure((size_t)spill_max * sizeof(am355_text_run))) ||
      !c->h_loc_runs.ensure((size_t)(N ? N : 1) * sizeof(am355_text_run)))
    return fail(c, AM355_E_NOMEM, "allocation failed (locate)");
  *runs = c->h_loc_runs.as<am355_text_run>();
  uint8_t* dp = c->d_loc.as<uint8_t>();
  uint32_t* dw = (uint32_t*)dp;
  uint4* d_ids = (uint4*)(dp + b_words);
  uint32_t* d_head = (uint32_t*)(dp + b_words + b_ids);
  uint32_t* d_cnt = d_head + b_arr / 4;
  uint32_t* d_pos = d_cnt + b_arr / 4;
  void* d_ws = dp + b_words + b_ids + 3 * b_arr;
  HIPCHK(c, hipMemsetAsync(dw, 0, LW_WORDS * 4, st));
  launch_text_check(o.recs, dw, st);
  c->n_locate_launches++;
  if (N) {
    const dim3 grid((N + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(kl_locate, grid, dim3(BLOCK), 0, st, o.recs, F, N, lead, dw, d_ids, d_head, d_cnt);
    exclusive_scan_u32(d_head, d_pos, N, dw + LW_RUNS, d_ws, st);
    AM355_LAUNCH_INDEPENDENT(kl_runs, grid, dim3(BLOCK), st, (const uint4*)d_ids, (const uint32_t*)d_head, (const uint32_t*)d_pos, (const uint32_t*)d_cnt, N, (const uint32_t*)dw,
                             c->h_loc_runs.as<am355_text_run>(), c->d_loc_runs.as<am355_text_run>());
    c->n_locate_launches += 3;
  }
  c->n_locate_launches++;
  // the one wait of the call: flag word, length, number of runs
  HIPCHK(c, c->text_sig.fetch(dw, LW_WORDS, 0, st));
  const uint32_t* hw = c->text_sig.words();
  const uint32_t lf = hw[LW_FLAGS];
  { int prc = text_premise_error(c, TC_LOCATE, lf, oi); if (prc) return prc; }
  *length = hw[LW_LENGTH];
  if (!fits || first + n > *length) { *past = true; return AM355_OK; }
  if (lf & LF_RANGE) return fail(c, AM355_E_DEVICE, "internal: the locate pass and the host disagree about the length of object %u", oi);
  const uint32_t nr = N ? hw[LW_RUNS] : 0u;
  if (nr > N || (N && !nr)) return fail(c, AM355_E_DEVICE, "internal: %u runs over %u elements", nr, N);
  { int src = spill_down(c, c->h_loc_runs.as<am355_text_run>(), (const am355_text_run*)c->d_loc_runs.as<am355_text_run>(), nr); if (src) return src; }
  *n_runs = nr;
  return AM355_OK;
}

int text_locate_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t first, uint64_t n, const am355_text_run** runs, uint32_t* n_runs,
                     uint64_t* length) {
  if (!c) return AM355_E_ARG;
  if (!runs || !n_runs || !length || (!obj_actor && actor_len)) return fail(c, AM355_E_ARG, "am355_text_locate: null argument");
  bool past = false;
  int rc = locate_core(c, "am355_text_locate", 0, obj_ctr, obj_actor, actor_len, first, n, 0, runs, n_runs, length, &past);
  if (rc) return rc;
  if (past)
    return fail(c, AM355_E_ARG, "elements [%llu, %llu + %llu) are out of bounds for a Text of length %llu", (unsigned long long)first, (unsigned long long)first,
                (unsigned long long)n, (unsigned long long)*length);
  return AM355_OK;
}

// actors of a request: raw ids, each once, the author first and the others in byte order (columnar.js:154-157), as the tables of
// am355_local_change
struct SpliceActors {
  std::vector<std::string> table;
  std::vector<uint32_t> off, rank;
  std::vector<uint8_t> bytes;
  SpliceActors(const std::string& me, std::vector<std::string> others) {
    std::sort(others.begin(), others.end());
    others.erase(std::unique(others.begin(), others.end()), others.end());
    table.push_back(me);
    for (const std::string& a : others)
      if (a != me) table.push_back(a);
    const uint32_t n = (uint32_t)table.size();
    off.assign(n + 1, 0); rank.assign(n, 0);
    for (uint32_t k = 0; k < n; k++) {
      bytes.insert(bytes.end(), table[k].begin(), table[k].end());
      off[k + 1] = (uint32_t)bytes.size();
      // (entries 1 .. are in byte order already: the author's rank is the number of them in front of it)
      rank[k] = k == 0 ? (uint32_t)(std::lower_bound(table.begin() + 1, table.end(), me) - (table.begin() + 1)) : (k - 1) + (table[k] > me ? 1u : 0u);
    }
  }
  uint32_t local(const std::string& a) const {
    for (uint32_t k = 0; k < table.size(); k++)
      if (table[k] == a) return k;
    return NONE32;
  }
};

// The request of a positional edit completed and applied: seq = the author's clock entry + 1, startOp = maxOp + 1, deps = the heads
// without the author's last change, which am355_apply_local_change adds itself (backend.js:73-81, 88-89). onto_nothing: seq 1, startOp 1, no deps.
int splice_apply(am355_ctx* c, const SpliceActors& act, const uint8_t* author, size_t author_len, int64_t time, const uint8_t* message, uint32_t message_len,
                 const uint8_t* strings, uint32_t strings_len, const std::vector<am355_local_op>& ops, const std::vector<am355_local_value>& values,
                 const std::vector<am355_local_pred>& preds, const uint8_t** change, size_t* len, bool onto_nothing = false) {
  am355_local_change lc{};
  lc.seq = 1;
  lc.start_op = 1;
  lc.time = time;
  lc.message = message; lc.message_len = message_len;
  std::vector<uint8_t> deps;
  if (!onto_nothing) {   // (a context without a state is Backend.init(): no clock, no heads, maxOp 0)
    uint32_t rank = 0;
    if (actor_rank_of(c, author, author_len, &rank))
      for (size_t k = 0; k < c->clock_actor.size(); k++)
        if (c->clock_actor[k] == rank) lc.seq = c->clock_seq[k] + 1;
    lc.start_op = c->max_op + 1;
    deps = c->heads;
    uint32_t last = NONE32;
    int rc;
    if (lc.seq > 1 && c->h_hashes.p && (rc = staged_change_of(c, author, author_len, lc.seq - 1, &last))) return rc;
    if (last != NONE32) {
      const uint8_t* h = c->h_hashes.as<uint8_t>() + 32 * (size_t)last;
      for (size_t k = 0; k + 32 <= deps.size(); k += 32)
        if (memcmp(&deps[k], h, 32) == 0) { deps.erase(deps.begin() + k, deps.begin() + k + 32); break; }
    }
  }
  lc.deps = deps.data(); lc.n_deps = (uint32_t)(deps.size() / 32);
  lc.n_actors = (uint32_t)act.table.size(); lc.actor_off = act.off.data(); lc.actor_bytes = act.bytes.data(); lc.actor_rank = act.rank.data();
  lc.strings = strings; lc.strings_len = strings_len;
  lc.ops = ops.data(); lc.n_ops = (uint32_t)ops.size();
  lc.values = values.data(); lc.n_values = (uint32_t)values.size();
  lc.preds = preds.data(); lc.n_preds = (uint32_t)preds.size();
  return apply_local_change_impl(c, &lc, change, len);
}

int text_splice_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t start, uint64_t deletions, const uint8_t* utf8,
                     const uint32_t* value_off, uint32_t n_values, const uint8_t* author, size_t author_len, int64_t time, const uint8_t* message, uint32_t message_len,
                     const uint8_t** change, size_t* len) {
  if (!c) return AM355_E_ARG;
  auto refused = [&](int code) { c->n_splice_refused++; return code; };
  if (!change || !len || (!obj_actor && actor_len) || !author || !author_len || (n_values && (!value_off || (!utf8 && value_off[n_values]))) || (!message && message_len))
    return refused(fail(c, AM355_E_ARG, "am355_text_splice: null argument"));
  for (uint32_t k = 0; k < n_values; k++)
    if (value_off[k + 1] < value_off[k]) return refused(fail(c, AM355_E_ARG, "am355_text_splice: value offsets out of order"));
  const TraceLap lap("text_splice:", 26);
  *change = nullptr; *len = 0;

  // ---- locate [start - 1, start + deletions): the insertion's reference element, then the deleted ones; on the state of the document's
  // rebuilt changes, whose clock, heads and max_op the request needs ----
  const uint32_t lead = start ? 1u : 0u;
  const am355_text_run* runs = nullptr;
  uint32_t n_runs = 0;
  uint64_t length = 0;
  bool past = false;
  const uint64_t q_first = start - lead, q_n = deletions + lead;
  const bool wraps = q_n < deletions || q_first + q_n < q_first;
  int rc = locate_core(c, "am355_text_splice", TO_CHANGE_STATE | TO_NO_QUEUE, obj_ctr, obj_actor, actor_len, wraps ? 0 : q_first, wraps ? 0 : q_n, lead, &runs, &n_runs, &length, &past);
  if (rc) return refused(rc);
  lap("located");
  if (wraps || past)   // context.js:444-446
    return refused(fail(c, AM355_E_ARG, "%llu deletions starting at index %llu are out of bounds for list of length %llu", (unsigned long long)deletions,
                        (unsigned long long)start, (unsigned long long)length));
  if (deletions == 0 && n_values == 0) { c->n_splice_served++; return AM355_OK; }   // context.js:447
  for (uint32_t r = lead; r < n_runs; r++)
    if (runs[r].flags & AM355_RUN_COUNTER) return refused(fail(c, AM355_E_INVALID, "Unsupported operation: deleting a counter from a list"));   // context.js:471
  if (lead && (!n_runs || runs[0].count != 1)) return refused(fail(c, AM355_E_DEVICE, "internal: the reference element of the insertion is not a run of its own"));

  // ---- the request (context.js:452-496 the deletions, :370-405 insertListItems) ----
  const uint32_t NA = (uint32_t)c->actors.size();
  for (uint32_t r = 0; r < n_runs; r++)
    if (runs[r].elem_actor >= NA || runs[r].pred_actor >= NA) return refused(fail(c, AM355_E_DEVICE, "internal: run %u names an actor outside the table", r));
  const std::string me((const char*)author, author_len), obj_a((const char*)obj_actor, actor_len);
  std::vector<std::string> others{obj_a};
  for (uint32_t r = 0; r < n_runs; r++) {
    if (r >= lead || n_values) others.push_back(c->actors[runs[r].elem_actor]);
    if (r >= lead) others.push_back(c->actors[runs[r].pred_actor]);
  }
  const SpliceActors act(me, others);
  std::vector<am355_local_op> ops;
  std::vector<am355_local_pred> preds;
  std::vector<am355_local_value> values;
  const uint32_t obj_local = act.local(obj_a);
  for (uint32_t r = lead; r < n_runs; r++) {
    am355_local_op op{};
    op.action = 3;   // del
    op.obj_actor = obj_local; op.obj_ctr = (uint32_t)obj_ctr;
    op.key_kind = AM355_LK_ELEM;
    op.elem_actor = act.local(c->actors[runs[r].elem_actor]); op.elem_ctr = runs[r].elem_ctr;
    op.multi = runs[r].count;
    op.pred_first = (uint32_t)preds.size(); op.pred_num = 1;
    preds.push_back(am355_local_pred{act.local(c->actors[runs[r].pred_actor]), runs[r].pred_ctr});
    ops.push_back(op);
  }
  if (n_values) {
    am355_local_op op{};
    op.action = 1;   // set
    op.obj_actor = obj_local; op.obj_ctr = (uint32_t)obj_ctr;
    if (lead) { op.key_kind = AM355_LK_ELEM; op.elem_actor = act.local(c->actors[runs[0].elem_actor]); op.elem_ctr = runs[0].elem_ctr; }
    else op.key_kind = AM355_LK_HEAD;
    op.flags = AM355_LOP_INSERT | (n_values > 1 ? AM355_LOP_VALUES : 0u);
    op.multi = n_values;
    op.pred_first = (uint32_t)preds.size();
    for (uint32_t k = 0; k < n_values; k++) values.push_back(am355_local_value{AM355_LV_UTF8, value_off[k], value_off[k + 1] - value_off[k], 0, 0});
    ops.push_back(op);
  }
  lap("request built");
  rc = splice_apply(c, act, author, author_len, time, message, message_len, utf8, n_values ? value_off[n_values] : 0u, ops, values, preds, change, len);
  lap("applied");
  if (rc) return refused(rc);
  c->n_splice_served++;
  return AM355_OK;
}

}  // namespace

extern "C" int am355_text_locate(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t first, uint64_t n, const am355_text_run** runs,
                                 uint32_t* n_runs, uint64_t* length) {
  return guarded(c, [&]() { return text_locate_impl(c, obj_ctr, obj_actor, actor_len, first, n, runs, n_runs, length); });
}
extern "C" int am355_text_splice(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t start, uint64_t deletions, const uint8_t* utf8,
                                 const uint32_t* value_off, uint32_t n_values, const uint8_t* author, size_t author_len, int64_t time, const uint8_t* message,
                                 uint32_t message_len, const uint8_t** change, size_t* len) {
  return guarded(c, [&]() {
    return text_splice_impl(c, obj_ctr, obj_actor, actor_len, start, deletions, utf8, value_off, n_values, author, author_len, time, message, message_len, change, len);
  });
}
extern "C" int am355_text_splice_calls(const am355_ctx* c, uint64_t out[3]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_splice_served;
  out[1] = c->n_splice_refused;
  out[2] = c->n_locate_launches;
  return AM355_OK;
}
extern "C" int am355_actor_of_rank(const am355_ctx* c, uint32_t rank, const uint8_t** bytes, size_t* len) {
  if (!c || !bytes || !len) return AM355_E_ARG;
  if (!c->replayed) return AM355_E_STATE;
  if (rank >= c->actors.size()) return AM355_E_ARG;
  *bytes = (const uint8_t*)c->actors[rank].data();
  *len = c->actors[rank].size();
  return AM355_OK;
}
extern "C" int am355_text_locate_limits(uint32_t out[3]) {
  if (!out) return AM355_E_ARG;
  out[0] = BLOCK; out[1] = scan_single_limit(); out[2] = LOCATE_PINNED_RUNS;
  return AM355_OK;
}
