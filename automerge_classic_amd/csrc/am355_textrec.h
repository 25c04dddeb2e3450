// What the calls on a Text object share (am355_text.hip: am355_object_text; am355_locate.hip: am355_text_locate, am355_text_splice;
// am355_position.hip: am355_text_position): the rule of the edit-record table with its proof, stated once as device helpers, and the
// host half of a call -- its opening (state, object lookup), the premise bits as errors, results that come down pinned-then-spill.
//
// THE RECORD TABLE (am355_ir_edit; a list object owns the records [edit_begin, edit_end) and the table ends with a sentinel record).
// Record k holds count_k = first_{k+1} - first_k values, the elements index_k .. index_k + count_k - 1. Record k + 1 either opens
// index_k + count_k or carries AM355_EDIT_UPDATE with index == index_k + count_k - 1 and replaces that one value: only the last value
// of a record can be overwritten, only by the record directly behind it. Why (am355_merge.hip list_edits_of, k_edit_runs, k_edit_pack):
//   (a) list_edits_of writes the edits of ONE element side by side at e, e + 1, ...: first the value that stands as its insert, then its
//       other visible values in ascending op id, each with flag bit 0 (update) and the element's own index. Every edit without the
//       update bit therefore opens a new index (the edit of the next visible element: index + 1), and every edit with it sits directly
//       behind an edit of the same index -- or, for an element that was reported as `remove` first (removed_first), at the head of the
//       element's edits, where it stands for the element itself.
//   (b) k_edit_runs lets an edit continue the record of the edit before it (bit 1 without bit 10) only if BOTH are `simple`: no update,
//       child or remove bit and row == element. An update edit is never simple: it always starts a record (head = 1) and the edit behind
//       it starts one too. So a record with the update bit holds exactly one value, and a record of several values holds inserts of
//       consecutive indexes index, index + 1, ..., index + count - 1.
//   (c) From (a) and (b): the only value of record k that another edit can share its index with is its last one (index + count - 1),
//       and the edit that does is the first edit behind the record: the head of record k + 1, carrying the update bit and that index.
//       A chain insert, update, update of one element is three records; each is overwritten by the next and the last one stands.
//   (d) AM355_EDIT_CONT records are records like any other here: they continue the multi-insert EDIT of the record in front (a new
//       type/length word or a gap in the arena), not its values; their index and ids are those of their first value (k_edit_pack).
//   (e) k_edit_pack gives every list object the records [edit_begin, edit_end) and nothing else, so "belongs to the same object" is
//       k + 1 < edit_end.
// THE IDS OF AN ELEMENT. For element j let hi be the LAST record with hi.index <= j. Then
//     elemId = (hi.elem_ctr + (j - hi.index), hi.elem_actor)        pred = (hi.id_ctr + (j - hi.index), hi.id_actor)
//   (f) k_edit_pack fills EVERY record, update records too, from the head edit e of the record: id_ctr / id_actor = the op id of the row
//       e_row[e] that carries the value, elem_ctr / elem_actor = the op id of e_elem[e], the element's insert row -- its elemId. An
//       update record therefore carries the element's elemId itself; a second search (the last record WITHOUT the update bit, for the
//       elemId) is not needed, and would be wrong for an element whose edits all carry the update bit (removed_first in list_edits_of:
//       no record without the bit has its index).
//   (g) A record of several values holds `simple` edits only (k_edit_runs): row == element for each, consecutive op ids of one actor,
//       consecutive indexes. So value i of the record has elemId == opId == (id_ctr + i, id_actor) and elem_ctr == id_ctr: both formulas
//       above count up together, which is apply_patch.js's multi-insert rule. A record whose head edit is not simple (an update, a child,
//       an insert whose own value is gone and whose first listed value is another row: e_row != e_elem) holds ONE value, j - hi.index is 0
//       and the record's two ids are the element's: the `insert` edit with opId != elemId, or the `update` edit that replaced it.
//   (h) hi is the last edit of j's index: records are in document order, the edits of one element stand side by side, and only the last
//       value of a record shares its index with the record behind (c) -- for an inner value of a record hi is the record itself, for
//       its last value the last update record behind it, if there is one.
// The element is a counter iff hi carries AM355_EDIT_COUNTER (a counter completed by increments, listed under its last increment) or
// hi is a plain value record whose type is COUNTER (val_tl & 15 == 8, columnar.js:47-48: a counter nobody has incremented yet is an
// ordinary `set` row to the engine, and `new Counter` to the frontend).
// The engine never builds a table that breaks the rule; rec_premises verifies it per record all the same before anything is searched:
// indexes that start at 0 and continue as stated, `first` words in order and inside the table, no `remove` record.
#pragma once
#include "am355_ctx.h"

namespace am355 {

struct TextRecs {   // the records of one object
  const am355_ir_edit* edit;   // the whole-document edit records
  uint32_t begin, R;           // the object's records [begin, begin + R)
  uint32_t n_values;           // values of the whole table (the `first` word of the sentinel record)
  __device__ __forceinline__ const am355_ir_edit& operator[](uint32_t k) const { return edit[begin + k]; }   // record k of the object (k == R: the one behind; the table ends with a sentinel)
};
// flag bits of a call's device words: the premises, which every call shares, and the first bit of a call's own
enum RecFlag : uint32_t { RF_TABLE = 1,    // the records do not continue each other as the rule needs, or name values outside the table
                          RF_REMOVE = 2,   // a `remove` record: an element that shows rows but no value
                          RF_CALL = 4 };
constexpr uint32_t LOCATE_PINNED_RUNS = 4096;   // items of a result a kernel writes straight into pinned host memory (runs: 96 KiB); the ones behind go to HBM and down in one copy

// values of record k (k < R). false, and 0 of them: its `first` words are out of order or past the table.
__device__ __forceinline__ bool rec_count(const TextRecs& t, uint32_t k, uint32_t& count) {
  const uint32_t first = t[k].first, next = t[k + 1].first;
  count = (next <= first || next > t.n_values) ? 0u : next - first;
  return count != 0;
}
// the record behind record k replaces its last value (c)
__device__ __forceinline__ bool rec_overwritten(const TextRecs& t, uint32_t k, uint32_t count) {
  return k + 1 < t.R && (t[k + 1].flags & AM355_EDIT_UPDATE) && t[k + 1].index == t[k].index + count - 1;
}
__device__ __forceinline__ bool rec_is_counter(const am355_ir_edit& rec) {
  return (rec.flags & AM355_EDIT_COUNTER) || (!(rec.flags & AM355_EDIT_CHILD) && (rec.val_tl & 15u) == 8u);
}
// The premises of record k: RF_TABLE | RF_REMOVE, 0 when it is as the rule says. The last record then leaves the object's length.
__device__ __forceinline__ uint32_t rec_premises(const TextRecs& t, uint32_t k, uint32_t& count, uint32_t& length) {
  const am355_ir_edit& rec = t[k];
  uint32_t err = 0;
  if (rec.flags & AM355_EDIT_REMOVE) err |= RF_REMOVE;
  if (!rec_count(t, k, count)) err |= RF_TABLE;
  if (k == 0 && rec.index != 0) err |= RF_TABLE;
  if ((rec.flags & AM355_EDIT_UPDATE) && count > 1) err |= RF_TABLE;   // (b)
  if (count && (uint64_t)rec.index + count > 0xffffffffull) err |= RF_TABLE;
  if (err) return err;
  if (k + 1 == t.R) { length = rec.index + count; return 0; }
  return t[k + 1].index == rec.index + count || rec_overwritten(t, k, count) ? 0u : (uint32_t)RF_TABLE;
}
// the last record with index <= j (indexes are non-decreasing: the check pass). Reads only records of [begin, begin + R), R >= 1.
__device__ __forceinline__ uint32_t rec_last_at(const TextRecs& t, uint32_t j) {
  uint32_t lo = 0, hi = t.R;   // t[lo].index <= j < t[hi].index (record 0 has index 0; hi == R: the end)
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (t[mid].index <= j) lo = mid; else hi = mid;
  }
  return lo;
}
// ids of element j by THE IDS OF AN ELEMENT above: {elemId ctr, elemId actor, id ctr, id actor} of its last edit; counter = rec_is_counter of it
__device__ __forceinline__ uint4 locate_ids(const TextRecs& t, uint32_t j, uint32_t& counter) {
  const am355_ir_edit& rec = t[rec_last_at(t, j)];
  const uint32_t d = j - rec.index;
  counter = rec_is_counter(rec) ? 1u : 0u;
  return uint4{rec.elem_ctr + d, rec.elem_actor, rec.id_ctr + d, rec.id_actor};
}
// where item i of a result goes: pinned[i] for i < LOCATE_PINNED_RUNS, else spill[i - LOCATE_PINNED_RUNS]
template <class T>
__device__ __forceinline__ T* pinned_or_spill(T* pinned, T* spill, uint32_t i) { return i < LOCATE_PINNED_RUNS ? pinned + i : spill + (i - LOCATE_PINNED_RUNS); }

// the check pass (am355_locate.hip kl_check) over t: words[0] |= the premise bits, words[1] = the length when there are none
void launch_text_check(const TextRecs& t, uint32_t* words, hipStream_t st);
// the check pass of the calls on a plain list (am355_list_locate.hip klist_check): the same words, and its own bit for an element without an insert
void launch_list_check(const TextRecs& t, uint32_t* words, hipStream_t st);

// device words of the lookup and of a read (d_text): what kt_find found, then the totals and the flag word of kt_sizes
enum TextWord { TW_INDEX = 0, TW_TYPE = 1, TW_BEGIN = 2, TW_END = 3, TW_BYTES = 4, TW_ELEMS = 5, TW_NONSTR = 6, TW_FLAGS = 7, TW_WORDS = 8 };
// One thread per object: the object with that id leaves its index, type and edit range -- or, maps != 0, its range of map records. (_root, index 0, has no id.)
static __global__ __launch_bounds__(BLOCK) void kt_find(const am355_ir_object* __restrict__ obj, uint32_t n_obj, uint32_t ctr, uint32_t actor, uint32_t maps, uint32_t* __restrict__ words) {
  const uint32_t i = gtid();
  if (i == 0 || i >= n_obj) return;
  if (obj[i].id_ctr != ctr || obj[i].id_actor != actor) return;
  words[TW_INDEX] = i;
  words[TW_TYPE] = obj[i].type;
  words[TW_BEGIN] = maps ? obj[i].map_begin : obj[i].edit_begin;
  words[TW_END] = maps ? obj[i].map_end : obj[i].edit_end;
}

}  // namespace am355

// ---- the host half ----
static inline int text_poll(am355_ctx* c) {   // (short copies and kernels: polled, not slept on -- fetch_ir_impl)
  hipError_t q;
  while ((q = hipStreamQuery(c->stream)) == hipErrorNotReady) {}
  if (q != hipSuccess) HIPCHK(c, q);
  return AM355_OK;
}

// items [LOCATE_PINNED_RUNS, n) of a result down from the spill array, behind the kernel that wrote them
template <class T>
static inline int spill_down(am355_ctx* c, T* host, const T* spill, uint32_t n) {
  if (n <= LOCATE_PINNED_RUNS) return AM355_OK;
  HIPCHK(c, hipMemcpyAsync(host + LOCATE_PINNED_RUNS, spill, (size_t)(n - LOCATE_PINNED_RUNS) * sizeof(T), hipMemcpyDeviceToHost, c->stream));
  return text_poll(c);
}

enum TextCall { TC_READ, TC_LOCATE, TC_POSITION };
// the premise bits of a call's flag word as that call's error (AM355_OK: none is set)
static inline int text_premise_error(am355_ctx* c, TextCall call, uint32_t flags, uint32_t oi) {
  const bool table = flags & RF_TABLE, remove = call != TC_READ && (flags & RF_REMOVE);   // (a read counts a `remove` record as nothing)
  if (remove && (call == TC_POSITION || !table))
    return fail(c, AM355_E_UNSUPPORTED, "a Text element that shows rows but no value (a `remove` record): positions through the patch");
  if (table && call == TC_READ) return fail(c, AM355_E_DEVICE, "internal: an edit record of object %u names values outside the tables", oi);
  if (table)
    return fail(c, AM355_E_DEVICE, "internal: the edit records of object %u do not continue each other%s", oi, call == TC_POSITION ? ", or their elements are not in document order" : "");
  return AM355_OK;
}

enum TextOpenFlag : uint32_t { TO_CHANGE_STATE = 1,   // a document context becomes the state of its rebuilt changes first (as am355_apply_local_change)
                               TO_NO_QUEUE = 2 };     // refused on a state with queued changes
struct TextObject { uint32_t index, actor_rank; TextRecs recs; };   // index in the object table | rank of the id's actor | its records
// The state a call `who` on an object needs (shared by the calls on a Text, a plain list and a map): replayed, not sharded, a document
// context turned into the state of its rebuilt changes and no queued changes where the flags ask for it.
static inline int call_open_state(am355_ctx* c, const char* who, uint32_t flags) {
  if (!c->replayed) return fail(c, AM355_E_STATE, "%s: a replayed state is needed", who);
  if (c->shard_world > 1) return fail(c, AM355_E_UNSUPPORTED, "%s on a sharded context", who);
  (void)hipSetDevice(c->device);
  if ((flags & TO_CHANGE_STATE) && c->staged && c->is_document) {
    int rc = document_to_change_state(c, [](const char*) {});
    if (rc) return rc;
    if (!c->replayed) return fail(c, AM355_E_STATE, "%s: a replayed state is needed", who);
  }
  if ((flags & TO_NO_QUEUE) && (!c->pending_change.empty() || c->n_pending)) return fail(c, AM355_E_UNSUPPORTED, "local change onto a state with queued changes: JS path");
  return AM355_OK;
}
// The object (obj_ctr, obj_actor), not _root: its index, the rank of its actor, its type and its range of edit records (maps: of map
// records) -- from the host's copy of the object table when it is the device's, else one launch over ir.obj (+ the launch that signals the
// four words; counted in *launches). No such object: AM355_E_ARG "no such object: <ctr>@<actor in hex>".
struct FoundObject { uint32_t index, actor_rank, type, begin, end; };
static inline int object_lookup(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, bool maps, uint64_t* launches, FoundObject& f) {
  hipStream_t st = c->stream;
  const uint32_t NO = c->counts.n_objects;
  auto no_such = [&]() {
    std::string id = std::to_string((unsigned long long)obj_ctr) + "@";
    for (size_t k = 0; k < actor_len; k++) { id.push_back("0123456789abcdef"[obj_actor[k] >> 4]); id.push_back("0123456789abcdef"[obj_actor[k] & 15]); }
    return fail(c, AM355_E_ARG, "no such object: %s", id.c_str());
  };
  uint32_t rank = 0;
  if (obj_ctr > 0xffffffffull || !actor_rank_of(c, obj_actor, actor_len, &rank)) return no_such();
  if (!c->d_text.ensure(TW_WORDS * 4) || !c->text_sig.ready()) return fail(c, AM355_E_NOMEM, "allocation failed (text)");
  uint32_t oi = NONE32, type = 0, b = 0, e = 0;
  if (c->h_tables_current && c->hir.objects && c->hir.n_objects == NO) {
    for (uint32_t i = 1; i < NO; i++)
      if (c->hir.objects[i].id_ctr == (uint32_t)obj_ctr && c->hir.objects[i].id_actor == rank) {
        const am355_ir_object& ho = c->hir.objects[i];
        oi = i; type = ho.type; b = maps ? ho.map_begin : ho.edit_begin; e = maps ? ho.map_end : ho.edit_end;
        break;
      }
  } else if (NO > 1) {
    uint32_t* dw = c->d_text.as<uint32_t>();
    HIPCHK(c, hipMemsetAsync(dw, 0xff, 4 * 4, st));
    AM355_LAUNCH_INDEPENDENT(kt_find, dim3((NO + BLOCK - 1) / BLOCK), dim3(BLOCK), st, (const am355_ir_object*)c->ir.obj, NO, (uint32_t)obj_ctr, rank, maps ? 1u : 0u, dw);
    *launches += 2;
    HIPCHK(c, c->text_sig.fetch(dw, 4, 0, st));
    const uint32_t* hw = c->text_sig.words();
    oi = hw[TW_INDEX]; type = hw[TW_TYPE]; b = hw[TW_BEGIN]; e = hw[TW_END];
  }
  if (oi == NONE32) return no_such();
  f = FoundObject{oi, rank, type, b, e};
  return AM355_OK;
}
// The opening of a call `who` on the Text (or, want_type 2, the plain list) (obj_ctr, obj_actor): the state it needs, the edit tables fresh, the object found.
static inline int text_open(am355_ctx* c, const char* who, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint32_t flags, uint64_t* launches, TextObject& o,
                            uint32_t want_type = 4) {   // (4: a Text; 2: a plain list)
  { int src = call_open_state(c, who, flags); if (src) return src; }
  { int frc = ensure_ir_fresh(c); if (frc) return frc; }   // (in-place list merges leave the edit tables stale: rebuilt once)
  const uint32_t NR = c->counts.n_erecs;
  const char* not_wanted = want_type == 4 ? "not a Text object" : "not a list object";
  if (obj_ctr == 0 && actor_len == 0) return fail(c, AM355_E_ARG, "%s", not_wanted);   // (_root: a map)
  FoundObject f;
  { int lrc = object_lookup(c, obj_ctr, obj_actor, actor_len, false, launches, f); if (lrc) return lrc; }
  if (f.type != want_type) return fail(c, AM355_E_ARG, "%s", not_wanted);
  if (f.begin > f.end || f.end > NR) return fail(c, AM355_E_DEVICE, "internal: edit range [%u, %u) of object %u outside the %u records", f.begin, f.end, f.index, NR);
  o.index = f.index; o.actor_rank = f.actor_rank;
  o.recs = TextRecs{(const am355_ir_edit*)c->ir.edit, f.begin, f.end - f.begin, c->counts.n_edits};
  return AM355_OK;
}
