// Positions of a plain list (makeList, object type 2) resolved to ids on the device (include/am355.h: am355_list_locate), and the
// positional edits built from them (am355_list_splice, am355_list_set): what the reference's frontend does in context.splice
// (frontend/context.js:441-502), insertListItems (:370-405) and setListIndex (:411-435) for list.deleteAt / list.insertAt / list[i] = v,
// without a frontend document. The difference to a Text (am355_locate.hip): an element of a list keeps EVERY conflicting value, and the
// pred of a deletion or an assignment names all of them.
//
// THE RULE (frontend/apply_patch.js:156-213 updateListObject, context.js:576-596 getPred / getElemId):
//   1. Element j has one elemId and the values of the `insert` / `multi-insert` edit that opens index j and of every `update` edit of index
//      j directly behind it; getPred returns the op ids of all of them, in the order of the edits (ascending op id); the list shows the last.
//   2. A deletion joins the one before it as multiOp iff both elements have exactly one pred, the elemId actors are equal with consecutive
//      counters and the pred actors are equal with consecutive counters (context.js:479-486).
//   3. A deleted element whose shown value is a Counter throws (context.js:455-471), and so does an assignment onto one (:421-423).
//
// ON THE RECORD TABLE (am355_textrec.h (a) - (h)): for element j let hi be the LAST record with hi.index <= j and lo the FIRST record
// whose last index (index + count - 1) is >= j; last indexes are non-decreasing like the indexes, so both are binary searches. With
// d = j - hi.index the elemId is (hi.elem_ctr + d, hi.elem_actor) by (f). lo == hi: one pred, (hi.id_ctr + d, hi.id_actor). Otherwise j is
// the last value of lo (c) and lo + 1 .. hi are its update records: the preds are the id of lo's last value, (lo.id_ctr + count - 1,
// lo.id_actor), then the ids of lo + 1 .. hi -- pred_num = hi - lo + 1, in ascending op id by (a). The shown value is hi's (h).
// ONE EXCEPTION, the reference's own: when lo is (part of) a `multi-insert` edit -- a record of several values, or an AM355_EDIT_CONT
// record -- the `update` edits behind it do not stand "directly behind an insert or update edit of their index" for updateListObject:
// its multi-insert branch does not look ahead, the first update takes the other branch and REPLACES the element's conflicts
// (apply_patch.js:187-190). The frontend's preds are then the update records' ids alone, pred_num = hi - lo, and that is what is
// reproduced. No frontend makes such a history (an assignment names every value it replaces, so a value that stands as its element's
// insert has no sibling); a hand-made `set` without pred onto an existing element does.
// What the rule does not cover is refused: an element whose FIRST record carries the update bit (removed_first in (a)) has no ELEM_IDS
// entry in the reference's frontend -- klist_check gives it a flag bit of its own beside the premises of rec_premises.
//
// Included at the end of am355_calls.hip, not compiled by itself.
#include "am355_textrec.h"

namespace am355 {

// device words of a call (d_lloc): the first four come down in the one wait of the call
enum ListWord { LIW_FLAGS = 0, LIW_LENGTH = 1, LIW_RUNS = 2, LIW_PREDS = 3, LIW_COUNTERS = 4, LIW_WORDS = 5 };
constexpr uint32_t LIF_RANGE = RF_CALL,            // the queried range reaches past the object's length
                   LIF_NO_ELEM = RF_CALL << 1,     // an element whose first record carries the update bit
                   LIF_PREDS = RF_CALL << 2;       // an element of more than LIST_MAX_PREDS values
constexpr uint32_t LIST_MAX_PREDS = 4096;          // (the bound am355_apply_local_change has for the preds of one op)

// Check pass, one thread per record of the object: the premises of the searches (rec_premises), and the element without an insert. The
// last record's thread leaves the length.
__global__ __launch_bounds__(BLOCK) void klist_check(TextRecs t, uint32_t* __restrict__ words) {
  const uint32_t k = gtid();
  if (k >= t.R) return;
  uint32_t count, length;
  uint32_t err = rec_premises(t, k, count, length);
  if (t[k].flags & AM355_EDIT_UPDATE) {   // an update record stands behind a value of its index, or it stands for an element that has no insert
    uint32_t before = 0;
    if (k == 0 || !rec_count(t, k - 1, before) || t[k - 1].index + before - 1 != t[k].index) err |= LIF_NO_ELEM;
  }
  if (err) atomicOr(&words[LIW_FLAGS], err);
  else if (k + 1 == t.R) words[LIW_LENGTH] = length;
}
void launch_list_check(const TextRecs& t, uint32_t* words, hipStream_t st) {
  AM355_LAUNCH_INDEPENDENT(klist_check, dim3((t.R + BLOCK - 1) / BLOCK), dim3(BLOCK), st, t, words);
}

// what the locate pass knows of one element
struct ListElem {
  uint4 ids;           // elemId ctr, elemId actor, first pred ctr, first pred actor
  uint32_t lo;         // the record of its first pred
  uint32_t pred_num;   // its values
  uint32_t counter;    // the shown value is a Counter
};
// Element j of t (j < length): the two searches. Reads only records of [begin, begin + R] (rec_count looks at the record behind).
__device__ __forceinline__ ListElem list_elem(const TextRecs& t, uint32_t j) {
  const uint32_t hi = rec_last_at(t, j);
  uint32_t a = 0, b = hi;   // the first record in [0, hi] whose last index is >= j (hi's is: j < length, and the record behind hi opens an index > j)
  while (a < b) {
    const uint32_t mid = a + ((b - a) >> 1);
    uint32_t count;
    rec_count(t, mid, count);
    if ((uint64_t)t[mid].index + count > j) b = mid; else a = mid + 1;   // (index + count - 1 >= j; a count of 0 -- a broken table -- never holds j)
  }
  const am355_ir_edit& rh = t[hi];
  const uint32_t d = j - rh.index;
  ListElem e;
  e.lo = a;
  e.pred_num = hi - a + 1;
  e.counter = rec_is_counter(rh) ? 1u : 0u;
  e.ids = uint4{rh.elem_ctr + d, rh.elem_actor, rh.id_ctr + d, rh.id_actor};
  if (a != hi) {
    uint32_t count;
    rec_count(t, a, count);
    if (count > 1 || (t[a].flags & AM355_EDIT_CONT)) {   // a multi-insert edit: the frontend keeps the updates' ids alone
      e.lo = a + 1;
      e.pred_num = hi - a;
    }
    e.ids.z = t[e.lo].id_ctr;   // (a record of one value, or an update record)
    e.ids.w = t[e.lo].id_actor;
  }
  return e;
}

// Locate, one thread per queried element first + i: its ids, the record of its first pred, pred_num, counter bit, and head[i] = 1 iff
// the element does not continue the one before it by rule 2. Element 0 is a head, and so is element `lead` (1: the range begins one
// element early -- the reference element of an insertion, which is no deletion; 0: no such element). The neighbour comes from LDS; the
// first thread of a workgroup searches for it again. head_preds[i] = pred_num of a head, 0 of the others: the second array of the scan.
__global__ __launch_bounds__(BLOCK) void klist_locate(TextRecs t, uint32_t first, uint32_t n, uint32_t lead, uint32_t* __restrict__ words, uint4* __restrict__ ids,
                                                      uint32_t* __restrict__ lo, uint32_t* __restrict__ pred_num, uint32_t* __restrict__ head,
                                                      uint32_t* __restrict__ head_preds, uint32_t* __restrict__ counter) {
  __shared__ uint4 s_ids[BLOCK];
  __shared__ uint32_t s_pn[BLOCK];
  const uint32_t i = gtid();
  const uint32_t length = words[LIW_LENGTH];   // (klist_check, the launch before; 0 when it found the table broken)
  const bool live = i < n && (uint64_t)first + i < length;
  ListElem me{uint4{0, 0, 0, 0}, 0, 0, 0};
  if (live) me = list_elem(t, first + i);
  s_ids[threadIdx.x] = me.ids;
  s_pn[threadIdx.x] = me.pred_num;
  __syncthreads();
  if (i >= n) return;
  uint32_t h = 0;
  if (!live) atomicOr(&words[LIW_FLAGS], (uint32_t)LIF_RANGE);
  else {
    h = 1;
    if (me.pred_num > LIST_MAX_PREDS) atomicOr(&words[LIW_FLAGS], (uint32_t)LIF_PREDS);
    if (i != 0 && i != lead && me.pred_num == 1) {
      uint4 p;
      uint32_t ppn;
      if (threadIdx.x) { p = s_ids[threadIdx.x - 1]; ppn = s_pn[threadIdx.x - 1]; }
      else { const ListElem b = list_elem(t, first + i - 1); p = b.ids; ppn = b.pred_num; }
      if (ppn == 1 && p.y == me.ids.y && p.x + 1 == me.ids.x && p.w == me.ids.w && p.z + 1 == me.ids.z) h = 0;
    }
    if (me.counter) atomicAdd(&words[LIW_COUNTERS], 1u);   // (counters inside a list are rare: no contention to speak of)
  }
  ids[i] = me.ids; lo[i] = me.lo; pred_num[i] = me.pred_num; head[i] = h; counter[i] = me.counter;
  head_preds[i] = h ? (me.pred_num > LIST_MAX_PREDS ? 0u : me.pred_num) : 0u;
}

// Compaction, one thread per queried element: a head writes its run -- elemId, the distance to the next head (binary search over the
// scanned head bits, as kl_runs), whether a counter is among its elements -- and its preds: the first one from the locate pass, the
// others the ids of the update records lo + 1 .. lo + pred_num - 1. Run r and pred p go where pinned_or_spill says; a pred at or past
// pred_cap (which the bound records + elements excludes) is not written and leaves RF_TABLE.
__global__ __launch_bounds__(BLOCK) void klist_runs(TextRecs t, const uint4* __restrict__ ids, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ pred_num,
                                                    const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ pred_pos,
                                                    const uint32_t* __restrict__ counter, uint32_t n, uint32_t pred_cap, uint32_t* __restrict__ words,
                                                    am355_list_run* __restrict__ pinned, am355_list_run* __restrict__ spill, am355_list_pred* __restrict__ pred_pinned,
                                                    am355_list_pred* __restrict__ pred_spill) {
  const uint32_t i = gtid();
  if (i >= n || !head[i]) return;
  const uint32_t r = pos[i];
  uint32_t a = i, b = n;   // pos[a] <= r + 1 < pos[b]: everything up to and including the next head has at most r + 1 heads in front
  while (b - a > 1) {
    const uint32_t mid = a + ((b - a) >> 1);
    if (pos[mid] <= r + 1) a = mid; else b = mid;
  }
  const uint32_t end = (a > i && head[a]) ? a : a + 1;   // the next head, or n
  uint32_t counters = 0;
  if (words[LIW_COUNTERS])
    for (uint32_t x = i; x < end; x++) counters |= counter[x];
  const uint4 me = ids[i];
  const uint32_t pn = pred_num[i] > LIST_MAX_PREDS ? 0u : pred_num[i], p0 = pred_pos[i];
  am355_list_run* out = pinned_or_spill(pinned, spill, r);
  out->elem_ctr = me.x; out->elem_actor = me.y;
  out->count = end - i;
  out->flags = counters ? AM355_RUN_COUNTER : 0u;
  out->pred_first = p0; out->pred_num = pn;
  if ((uint64_t)p0 + pn > pred_cap || (pn > 1 && (uint64_t)lo[i] + pn > t.R)) { atomicOr(&words[LIW_FLAGS], (uint32_t)RF_TABLE); return; }
  for (uint32_t q = 0; q < pn; q++) {
    am355_list_pred* pp = pinned_or_spill(pred_pinned, pred_spill, p0 + q);
    if (q == 0) { pp->actor = me.w; pp->ctr = me.z; }
    else { const am355_ir_edit& rec = t[lo[i] + q]; pp->actor = rec.id_actor; pp->ctr = rec.id_ctr; }
  }
}

}  // namespace am355

namespace {

struct ListLocated {
  const am355_list_run* runs = nullptr;
  const am355_list_pred* preds = nullptr;
  uint32_t n_runs = 0, n_preds = 0;
  uint64_t length = 0;
  bool past = false;   // the range reaches past the length (no runs then)
};

// the flag word of a list call as its error (AM355_OK: nothing is set that forbids an answer)
int list_premise_error(am355_ctx* c, uint32_t flags, uint32_t oi) {
  if (flags & RF_TABLE) return fail(c, AM355_E_DEVICE, "internal: the edit records of object %u do not continue each other", oi);
  if (flags & RF_REMOVE) return fail(c, AM355_E_UNSUPPORTED, "a list element that shows rows but no value (a `remove` record): positions through the patch");
  if (flags & LIF_NO_ELEM) return fail(c, AM355_E_UNSUPPORTED, "a list element whose first edit is an `update` (no elemId in the frontend): positions through the patch");
  if (flags & LIF_PREDS) return fail(c, AM355_E_UNSUPPORTED, "a list element of more than %u conflicting values", LIST_MAX_PREDS);
  return AM355_OK;
}

// What the three calls share: the runs and preds of [first, first + n) of the list, its length. lead: see klist_locate.
int list_locate_core(am355_ctx* c, const char* who, uint32_t open_flags, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t first, uint64_t n, uint32_t lead,
                     ListLocated& out) {
  TextObject o;
  { int orc = text_open(c, who, obj_ctr, obj_actor, actor_len, open_flags, &c->n_list_launches, o, 2); if (orc) return orc; }
  hipStream_t st = c->stream;
  const uint32_t R = o.recs.R, oi = o.index;
  out = ListLocated();
  if (!c->h_lloc_runs.ensure(sizeof(am355_list_run)) || !c->h_lloc_preds.ensure(sizeof(am355_list_pred))) return fail(c, AM355_E_NOMEM, "host allocation failed (list locate)");
  out.runs = c->h_lloc_runs.as<am355_list_run>();
  out.preds = c->h_lloc_preds.as<am355_list_pred>();
  if (R == 0) {   // an empty list: nothing to launch
    out.past = first + n > 0 || first + n < first;
    return AM355_OK;
  }
  // (a range the 32-bit positions cannot hold lies past every list; the length is still wanted)
  const bool fits = first <= 0xffffffffull && n <= 0xffffffffull && first + n <= 0xffffffffull;
  const uint32_t N = fits ? (uint32_t)n : 0u, F = fits ? (uint32_t)first : 0u;
  // every pred of the range is a record of the object or the one value of an element: at most R + N of them
  const uint64_t cap64 = (uint64_t)N + R;
  if (cap64 > 0xffffffffull) return fail(c, AM355_E_UNSUPPORTED, "%s: more than 2^32 preds possible", who);
  const uint32_t pred_cap = N ? (uint32_t)cap64 : 0u;
  // words | ids | lo, pred_num, head, head_preds, counter, pos, pred_pos | scan workspace
  const size_t b_words = carve_size(LIW_WORDS, 4), b_ids = carve_size(N, 16), b_arr = carve_size(N, 4), b_ws = carve_round(scan_workspace_bytes(N ? N : 1));
  const uint32_t spill_runs = N > LOCATE_PINNED_RUNS ? N - LOCATE_PINNED_RUNS : 0u, spill_preds = pred_cap > LOCATE_PINNED_RUNS ? pred_cap - LOCATE_PINNED_RUNS : 0u;
  if (!c->d_lloc.ensure(b_words + b_ids + 7 * b_arr + b_ws) || (spill_runs && !c->d_lloc_runs.ensure((size_t)spill_runs * sizeof(am355_list_run))) ||
      (spill_preds && !c->d_lloc_preds.ensure((size_t)spill_preds * sizeof(am355_list_pred))) || !c->h_lloc_runs.ensure((size_t)(N ? N : 1) * sizeof(am355_list_run)) ||
      !c->h_lloc_preds.ensure((size_t)(pred_cap ? pred_cap : 1) * sizeof(am355_list_pred)))
    return fail(c, AM355_E_NOMEM, "allocation failed (list locate)");
  out.runs = c->h_lloc_runs.as<am355_list_run>();
  out.preds = c->h_lloc_preds.as<am355_list_pred>();
  uint8_t* dp = c->d_lloc.as<uint8_t>();
  uint32_t* dw = (uint32_t*)dp;
  uint4* d_ids = (uint4*)(dp + b_words);
  uint32_t* arr = (uint32_t*)(dp + b_words + b_ids);
  const size_t step = b_arr / 4;
  uint32_t *d_lo = arr, *d_pn = arr + step, *d_head = arr + 2 * step, *d_hp = arr + 3 * step, *d_cnt = arr + 4 * step, *d_pos = arr + 5 * step, *d_ppos = arr + 6 * step;
  void* d_ws = dp + b_words + b_ids + 7 * b_arr;
  HIPCHK(c, hipMemsetAsync(dw, 0, LIW_WORDS * 4, st));
  launch_list_check(o.recs, dw, st);
  c->n_list_launches++;
  if (N) {
    const dim3 grid((N + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(klist_locate, grid, dim3(BLOCK), 0, st, o.recs, F, N, lead, dw, d_ids, d_lo, d_pn, d_head, d_hp, d_cnt);
    exclusive_scan2_u32(d_head, d_pos, dw + LIW_RUNS, d_hp, d_ppos, dw + LIW_PREDS, N, d_ws, st);
    AM355_LAUNCH_INDEPENDENT(klist_runs, grid, dim3(BLOCK), st, o.recs, (const uint4*)d_ids, (const uint32_t*)d_lo, (const uint32_t*)d_pn, (const uint32_t*)d_head,
                             (const uint32_t*)d_pos, (const uint32_t*)d_ppos, (const uint32_t*)d_cnt, N, pred_cap, dw, c->h_lloc_runs.as<am355_list_run>(),
                             c->d_lloc_runs.as<am355_list_run>(), c->h_lloc_preds.as<am355_list_pred>(), c->d_lloc_preds.as<am355_list_pred>());
    c->n_list_launches += 3;
  }
  c->n_list_launches++;
  // the one wait of the call: flag word, length, number of runs, number of preds
  HIPCHK(c, c->text_sig.fetch(dw, 4, 0, st));
  const uint32_t* hw = c->text_sig.words();
  const uint32_t lf = hw[LIW_FLAGS];
  { int prc = list_premise_error(c, lf, oi); if (prc) return prc; }
  out.length = hw[LIW_LENGTH];
  if (!fits || first + n > out.length) { out.past = true; return AM355_OK; }
  if (lf & LIF_RANGE) return fail(c, AM355_E_DEVICE, "internal: the locate pass and the host disagree about the length of object %u", oi);
  const uint32_t nr = N ? hw[LIW_RUNS] : 0u, np = N ? hw[LIW_PREDS] : 0u;
  if (nr > N || (N && !nr) || np < nr || np > pred_cap) return fail(c, AM355_E_DEVICE, "internal: %u runs and %u preds over %u elements", nr, np, N);
  { int src = spill_down(c, c->h_lloc_runs.as<am355_list_run>(), (const am355_list_run*)c->d_lloc_runs.as<am355_list_run>(), nr); if (src) return src; }
  { int src = spill_down(c, c->h_lloc_preds.as<am355_list_pred>(), (const am355_list_pred*)c->d_lloc_preds.as<am355_list_pred>(), np); if (src) return src; }
  // every index the host follows is checked before it is used: the preds of a run lie in the array, actors in the table
  const uint32_t NA = (uint32_t)c->actors.size();
  for (uint32_t r = 0; r < nr; r++) {
    const am355_list_run& run = out.runs[r];
    if (run.elem_actor >= NA || !run.count || !run.pred_num || (uint64_t)run.pred_first + run.pred_num > np || (run.count > 1 && run.pred_num != 1))
      return fail(c, AM355_E_DEVICE, "internal: run %u of object %u is not a run", r, oi);
  }
  for (uint32_t p = 0; p < np; p++)
    if (out.preds[p].actor >= NA) return fail(c, AM355_E_DEVICE, "internal: pred %u names an actor outside the table", p);
  out.n_runs = nr; out.n_preds = np;
  return AM355_OK;
}

int list_locate_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t first, uint64_t n, const am355_list_run** runs, uint32_t* n_runs,
                     const am355_list_pred** preds, uint32_t* n_preds, uint64_t* length) {
  if (!c) return AM355_E_ARG;
  if (!runs || !n_runs || !preds || !n_preds || !length || (!obj_actor && actor_len)) return fail(c, AM355_E_ARG, "am355_list_locate: null argument");
  ListLocated l;
  int rc = list_locate_core(c, "am355_list_locate", 0, obj_ctr, obj_actor, actor_len, first, n, 0, l);
  *runs = l.runs; *n_runs = l.n_runs; *preds = l.preds; *n_preds = l.n_preds; *length = l.length;
  if (rc) return rc;
  if (l.past)
    return fail(c, AM355_E_ARG, "elements [%llu, %llu + %llu) are out of bounds for a list of length %llu", (unsigned long long)first, (unsigned long long)first,
                (unsigned long long)n, (unsigned long long)l.length);
  return AM355_OK;
}

// the class of a value for insertListItems' "all datatypes the same" (context.js:378-385): strings, booleans and null carry none
uint32_t list_value_class(uint32_t tag) {
  return tag == AM355_LV_NULL || tag == AM355_LV_FALSE || tag == AM355_LV_TRUE || tag == AM355_LV_UTF8 ? 0u : tag + 1;
}

// The ops of one positional call in the making: actors by their raw ids until the table is known.
struct ListRequest {
  am355_ctx* c;
  std::string me, obj_a;
  uint32_t obj_ctr;
  struct Op { am355_local_op op; std::string elem; std::vector<std::pair<std::string, uint32_t>> preds; };
  std::vector<Op> ops;
  std::vector<am355_local_value> values;
  uint64_t next_op;   // nextOpNum (context.js:29-46)
  void add(Op&& o) {
    next_op += o.op.multi;
    ops.push_back(std::move(o));
  }
  // `del` / assignment target: element `at` of a run with all its preds (a run of several elements has one pred each: ctr + at)
  Op on_run(const ListLocated& l, const am355_list_run& run, uint32_t action) {
    Op o{};
    o.op.action = action;
    o.op.key_kind = AM355_LK_ELEM;
    o.op.elem_ctr = run.elem_ctr;
    o.elem = c->actors[run.elem_actor];
    o.op.multi = 1;
    for (uint32_t q = 0; q < run.pred_num; q++) o.preds.emplace_back(c->actors[l.preds[run.pred_first + q].actor], l.preds[run.pred_first + q].ctr);
    return o;
  }
  // insertListItems (context.js:370-405) behind element (ref_ctr, ref_actor), or _head (ref == nullptr)
  void insert(const am355_list_run* ref, const am355_local_value* v, uint32_t n) {
    if (!n) return;
    bool same = true;
    for (uint32_t k = 1; k < n; k++) same = same && list_value_class(v[k].tag) == list_value_class(v[0].tag);
    Op o{};
    o.op.action = 1;   // set
    if (ref) { o.op.key_kind = AM355_LK_ELEM; o.op.elem_ctr = ref->elem_ctr; o.elem = c->actors[ref->elem_actor]; }
    else o.op.key_kind = AM355_LK_HEAD;
    if (same && n > 1) {
      o.op.flags = AM355_LOP_INSERT | AM355_LOP_VALUES;
      o.op.multi = n;
      o.op.val_first = (uint32_t)values.size();
      values.insert(values.end(), v, v + n);
      add(std::move(o));
      return;
    }
    for (uint32_t k = 0; k < n; k++) {
      Op s = o;
      if (k) { s.op.key_kind = AM355_LK_ELEM; s.op.elem_ctr = (uint32_t)(next_op - 1); s.elem = me; }   // the element the op before made
      s.op.flags = AM355_LOP_INSERT;
      s.op.multi = 1;
      s.op.val_first = (uint32_t)values.size();
      values.push_back(v[k]);
      add(std::move(s));
    }
  }
  int apply(const uint8_t* author, size_t author_len, int64_t time, const uint8_t* message, uint32_t message_len, const uint8_t* strings, uint32_t strings_len,
            const uint8_t** change, size_t* len) {
    if (next_op > 0xffffffffull) return fail(c, AM355_E_UNSUPPORTED, "counters beyond 2^32");
    std::vector<std::string> others{obj_a};
    for (const Op& o : ops) {
      if (o.op.key_kind == AM355_LK_ELEM) others.push_back(o.elem);
      for (const auto& p : o.preds) others.push_back(p.first);
    }
    const SpliceActors act(me, others);
    std::vector<am355_local_op> flat;
    std::vector<am355_local_pred> preds;
    const uint32_t obj_local = act.local(obj_a);
    for (const Op& o : ops) {
      am355_local_op op = o.op;
      op.obj_actor = obj_local; op.obj_ctr = obj_ctr;
      if (op.key_kind == AM355_LK_ELEM) op.elem_actor = act.local(o.elem);
      op.pred_first = (uint32_t)preds.size(); op.pred_num = (uint32_t)o.preds.size();
      for (const auto& p : o.preds) preds.push_back(am355_local_pred{act.local(p.first), p.second});
      flat.push_back(op);
    }
    return splice_apply(c, act, author, author_len, time, message, message_len, strings, strings_len, flat, values, preds, change, len);
  }
};

bool list_values_ok(const am355_local_value* values, uint32_t n, uint32_t strings_len) {
  for (uint32_t k = 0; k < n; k++)
    if (values[k].tag == AM355_LV_UTF8 && ((uint64_t)values[k].off + values[k].len > strings_len)) return false;
  return true;
}

int list_splice_impl(am355_ctx* c, const char* who, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t start, uint64_t deletions,
                     const am355_local_value* values, uint32_t n_values, const uint8_t* strings, uint32_t strings_len, const uint8_t* author, size_t author_len, int64_t time,
                     const uint8_t* message, uint32_t message_len, const uint8_t** change, size_t* len) {
  if (!c) return AM355_E_ARG;
  auto refused = [&](int code) { c->n_list_refused++; return code; };
  if (!change || !len || (!obj_actor && actor_len) || !author || !author_len || (n_values && !values) || (!strings && strings_len) || (!message && message_len))
    return refused(fail(c, AM355_E_ARG, "%s: null argument", who));
  if (!list_values_ok(values, n_values, strings_len)) return refused(fail(c, AM355_E_ARG, "%s: a string value outside `strings`", who));
  const TraceLap lap("list_splice:", 26);
  *change = nullptr; *len = 0;
  // ---- locate [start - 1, start + deletions): the insertion's reference element, then the deleted ones ----
  const uint32_t lead = start ? 1u : 0u;
  ListLocated l;
  const uint64_t q_first = start - lead, q_n = deletions + lead;
  const bool wraps = q_n < deletions || q_first + q_n < q_first;
  int rc = list_locate_core(c, who, TO_CHANGE_STATE | TO_NO_QUEUE, obj_ctr, obj_actor, actor_len, wraps ? 0 : q_first, wraps ? 0 : q_n, lead, l);
  if (rc) return refused(rc);
  lap("located");
  if (wraps || l.past)   // context.js:444-446
    return refused(fail(c, AM355_E_ARG, "%llu deletions starting at index %llu are out of bounds for list of length %llu", (unsigned long long)deletions,
                        (unsigned long long)start, (unsigned long long)l.length));
  if (deletions == 0 && n_values == 0) { c->n_list_served++; return AM355_OK; }   // context.js:447
  for (uint32_t r = lead; r < l.n_runs; r++)
    if (l.runs[r].flags & AM355_RUN_COUNTER) return refused(fail(c, AM355_E_INVALID, "Unsupported operation: deleting a counter from a list"));   // context.js:471
  if (lead && (!l.n_runs || l.runs[0].count != 1)) return refused(fail(c, AM355_E_DEVICE, "internal: the reference element of the insertion is not a run of its own"));
  // ---- the request (context.js:452-496 the deletions, :370-405 insertListItems) ----
  ListRequest rq{c, std::string((const char*)author, author_len), std::string((const char*)obj_actor, actor_len), (uint32_t)obj_ctr, {}, {}, c->max_op + 1};
  for (uint32_t r = lead; r < l.n_runs; r++) {
    ListRequest::Op o = rq.on_run(l, l.runs[r], 3);   // del
    o.op.multi = l.runs[r].count;
    rq.add(std::move(o));
  }
  rq.insert(lead ? &l.runs[0] : nullptr, values, n_values);
  lap("request built");
  rc = rq.apply(author, author_len, time, message, message_len, strings, strings_len, change, len);
  lap("applied");
  if (rc) return refused(rc);
  c->n_list_served++;
  return AM355_OK;
}

constexpr uint64_t LIST_SET_MAX_NULLS = 1u << 20;   // list[index] = v far past the end: that many nulls at the most

int list_set_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t index, const am355_local_value* value, const uint8_t* strings,
                  uint32_t strings_len, const uint8_t* author, size_t author_len, int64_t time, const uint8_t* message, uint32_t message_len, const uint8_t** change,
                  size_t* len) {
  if (!c) return AM355_E_ARG;
  auto refused = [&](int code) { c->n_list_refused++; return code; };
  if (!change || !len || (!obj_actor && actor_len) || !author || !author_len || !value || (!strings && strings_len) || (!message && message_len))
    return refused(fail(c, AM355_E_ARG, "am355_list_set: null argument"));
  if (!list_values_ok(value, 1, strings_len)) return refused(fail(c, AM355_E_ARG, "am355_list_set: a string value outside `strings`"));
  *change = nullptr; *len = 0;
  ListLocated l;
  int rc = list_locate_core(c, "am355_list_set", TO_CHANGE_STATE | TO_NO_QUEUE, obj_ctr, obj_actor, actor_len, index, 1, 0, l);
  if (rc) return refused(rc);
  if (l.past) {   // context.js:416-420: nulls up to the index, then the value, spliced in at the end (a second locate: of the last element)
    const uint64_t nulls = index - l.length;
    if (nulls > LIST_SET_MAX_NULLS) return refused(fail(c, AM355_E_UNSUPPORTED, "am355_list_set: index %llu lies more than %llu elements past the end", (unsigned long long)index, (unsigned long long)LIST_SET_MAX_NULLS));
    std::vector<am355_local_value> values((size_t)nulls, am355_local_value{AM355_LV_NULL, 0, 0, 0, 0});
    values.push_back(*value);
    return list_splice_impl(c, "am355_list_set", obj_ctr, obj_actor, actor_len, l.length, 0, values.data(), (uint32_t)values.size(), strings, strings_len, author, author_len, time,
                            message, message_len, change, len);
  }
  if (l.n_runs != 1 || l.runs[0].count != 1) return refused(fail(c, AM355_E_DEVICE, "internal: one element located as %u runs", l.n_runs));
  if (l.runs[0].flags & AM355_RUN_COUNTER)   // context.js:421-423
    return refused(fail(c, AM355_E_INVALID, "Cannot overwrite a Counter object; use .increment() or .decrement() to change its value."));
  ListRequest rq{c, std::string((const char*)author, author_len), std::string((const char*)obj_actor, actor_len), (uint32_t)obj_ctr, {}, {}, c->max_op + 1};
  ListRequest::Op o = rq.on_run(l, l.runs[0], 1);   // set, insert: false
  o.op.val_first = 0;
  rq.values.push_back(*value);
  rq.add(std::move(o));
  rc = rq.apply(author, author_len, time, message, message_len, strings, strings_len, change, len);
  if (rc) return refused(rc);
  c->n_list_served++;
  return AM355_OK;
}

}  // namespace

extern "C" int am355_list_locate(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t first, uint64_t n, const am355_list_run** runs,
                                 uint32_t* n_runs, const am355_list_pred** preds, uint32_t* n_preds, uint64_t* length) {
  return guarded(c, [&]() { return list_locate_impl(c, obj_ctr, obj_actor, actor_len, first, n, runs, n_runs, preds, n_preds, length); });
}
extern "C" int am355_list_splice(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t start, uint64_t deletions, const am355_local_value* values,
                                 uint32_t n_values, const uint8_t* strings, uint32_t strings_len, const uint8_t* author, size_t author_len, int64_t time, const uint8_t* message,
                                 uint32_t message_len, const uint8_t** change, size_t* len) {
  return guarded(c, [&]() {
    return list_splice_impl(c, "am355_list_splice", obj_ctr, obj_actor, actor_len, start, deletions, values, n_values, strings, strings_len, author, author_len, time, message,
                            message_len, change, len);
  });
}
extern "C" int am355_list_set(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint64_t index, const am355_local_value* value, const uint8_t* strings,
                              uint32_t strings_len, const uint8_t* author, size_t author_len, int64_t time, const uint8_t* message, uint32_t message_len, const uint8_t** change,
                              size_t* len) {
  return guarded(c, [&]() { return list_set_impl(c, obj_ctr, obj_actor, actor_len, index, value, strings, strings_len, author, author_len, time, message, message_len, change, len); });
}
extern "C" int am355_list_splice_calls(const am355_ctx* c, uint64_t out[3]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_list_served;
  out[1] = c->n_list_refused;
  out[2] = c->n_list_launches;
  return AM355_OK;
}
extern "C" int am355_list_locate_limits(uint32_t out[3]) {
  if (!out) return AM355_E_ARG;
  out[0] = BLOCK; out[1] = scan_single_limit(); out[2] = LOCATE_PINNED_RUNS;
  return AM355_OK;
}
