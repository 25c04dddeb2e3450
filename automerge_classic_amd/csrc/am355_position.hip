// ElemIds of a Text resolved to positions on the device (include/am355.h: am355_text_position): the inverse of am355_text_locate, and
// the one question the whole-document patch cannot answer -- where a DELETED element stood. A caller that keeps a caret, a selection
// or a comment anchor alive while remote changes arrive names the place by elemId, the only stable name an RGA text has.
//
// THE RULE (pinned to the reference by a probe: a change of a fresh actor with startOp = maxOp + 1, deps = heads and one op
// {set, insert, elemId: X}; its op id is the greatest, so it lands directly behind X, in front of X's other children, and the patch
// reports it at index = the caret position behind X):
//   VISIBLE  X is an element of the Text: its index, text.getElemId(position) === X.
//   DELETED  X was inserted into this Text and shows no value any more: the number of visible elements in front of it in document order.
//   UNKNOWN  no applied change inserted such an element into this object.
// In both known cases the caret behind X is position + (status == VISIBLE).
//
// ONE MECHANISM FOR BOTH: a search by position in the stored list order. MergeBufs.order holds every insert row of every list, deleted
// ones too, in document order; pos_of[row] (resorder_positions) is its inverse. The edit records of the object ([edit_begin, edit_end),
// am355_textrec.h (f) - (h)) are in document order and every record carries its head element's elemId, so
//     rec_pos[k] = pos_of[row_of(record k's elemId)]
// is non-decreasing (an update record repeats the position of the value it replaces). For a queried element at position p:
//   hi = the LAST record with rec_pos[hi] <= p; none: nothing visible stands in front of it -- DELETED at 0;
//   inside hi, whose values are the elements (elem_ctr + i, elem_actor), i < count: d = the number of them whose position is < p, by
//   binary search over pos_of[row_of(...)]. The elements of one record are NOT taken to be adjacent in `order`: a tombstone of another
//   actor can stand between two of them. If one of them has position == p the element is VISIBLE at hi.index + d, else DELETED there.
// Why the last such record is the right one for a visible element: it lies in some record k at offset i, so rec_pos[k] <= p; the
// record behind has a greater position unless it is the update that replaces exactly this element, whose one value is the element.
// kp_heads builds rec_pos in one parallel pass and checks the premises of the record table (rec_premises) beside it, so a query's chain of dependent loads is
// log2(records) + log2(count) * log2(spans) instead of log2(records) * log2(spans).
// Every row and every position read is checked against the row count and the list length before it is used as an index.
//
// Included at the end of am355_calls.hip, not compiled by itself.
#include "am355_textrec.h"
#include "am355_rows.h"
#include "am355_resorder.h"

namespace am355 {

// device words of a call (d_posq)
enum PosWord { PW_FLAGS = 0, PW_LENGTH = 1, PW_WORDS = 2 };
constexpr uint32_t PF_RANGE = RF_CALL;   // flag bit of a call: a row or a position read for a query lies outside the tables (RF_TABLE here also: the head elements of the records are not in document order)

struct PosQuery {
  TextRecs recs;               // the object's records
  const uint32_t* pos_of;      // [rows] position in `order` of every list insert row
  uint32_t n_list;             // entries of `order`
  uint32_t obj_ctr, obj_actor; // the Text
};

// position of an insert row of the queried object, NONE32 when the id names no such row. *bad: the row is one, but its position is not
// what `order` says (nothing is read out of range either way).
__device__ __forceinline__ uint32_t pos_of_elem(const MergeBufs& b, const PosQuery& q, uint32_t actor, uint32_t ctr, bool& bad) {
  const uint32_t row = row_of(b, actor, ctr);
  if (row == NONE32 || row >= b.n_ops) return NONE32;
  const uint8_t kind = b.kind[row];
  if (!b.ops.insert[row] || (kind != K_LIST_INS && kind != K_LIST_INS_VIS)) return NONE32;
  if (b.ops.obj_ctr[row] != q.obj_ctr || b.ops.obj_actor[row] != q.obj_actor) return NONE32;
  const uint32_t p = q.pos_of[row];
  if (p >= q.n_list || b.order[p] != row) { bad = true; return NONE32; }
  return p;
}

// Heads pass, one thread per record of the object: the premises (rec_premises), rec_pos[k], and rec_pos[k] <= rec_pos[k + 1].
// The last record's thread leaves the length.
__global__ __launch_bounds__(BLOCK) void kp_heads(MergeBufs b, PosQuery q, uint32_t* __restrict__ rec_pos, uint32_t* __restrict__ words) {
  const uint32_t k = gtid();
  if (k >= q.recs.R) return;
  const am355_ir_edit& rec = q.recs[k];
  uint32_t count, length;
  uint32_t err = rec_premises(q.recs, k, count, length);
  if (count && (uint64_t)rec.elem_ctr + count > 0xffffffffull) err |= RF_TABLE;
  bool bad = false;
  const uint32_t p = pos_of_elem(b, q, rec.elem_actor, rec.elem_ctr, bad);
  if (p == NONE32) err |= RF_TABLE;   // (the head element of a record is an insert row of this object)
  rec_pos[k] = p;
  if (!err) {
    if (k + 1 < q.recs.R) {
      const am355_ir_edit& nxt = q.recs[k + 1];
      const uint32_t pn = pos_of_elem(b, q, nxt.elem_actor, nxt.elem_ctr, bad);
      if (pn == NONE32 || pn < p) err |= RF_TABLE;
    } else {
      words[PW_LENGTH] = length;
    }
  }
  if (err) atomicOr(&words[PW_FLAGS], err);
}

// Resolve, one thread per query: see the header. Result i goes where pinned_or_spill says.
__global__ __launch_bounds__(BLOCK) void kp_resolve(MergeBufs b, PosQuery q, const uint32_t* __restrict__ rec_pos, const am355_elem_id* __restrict__ ids, uint32_t n,
                                                    uint32_t* __restrict__ words, am355_elem_pos* __restrict__ pinned, am355_elem_pos* __restrict__ spill) {
  const uint32_t i = gtid();
  if (i >= n) return;
  const am355_elem_id id = ids[i];
  uint32_t status = AM355_POS_UNKNOWN, position = 0;
  bool bad = false;
  const uint32_t p = pos_of_elem(b, q, id.actor, id.ctr, bad);
  if (p != NONE32) {
    status = AM355_POS_DELETED;
    uint32_t lo = 0, hi = q.recs.R;   // records [0, lo) have rec_pos <= p, records [hi, R) a greater one
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (rec_pos[mid] <= p) lo = mid + 1; else hi = mid;
    }
    if (lo) {
      const am355_ir_edit& rec = q.recs[lo - 1];
      uint32_t count;
      (void)rec_count(q.recs, lo - 1, count);   // (kp_heads has checked the words; a broken table fails the call)
      uint32_t a = 0, e = count;   // elements [0, a) of the record stand in front of p, elements [e, count) at or behind it
      bool found = false;
      while (a < e && !bad) {
        const uint32_t mid = a + ((e - a) >> 1);
        const uint32_t pm = pos_of_elem(b, q, rec.elem_actor, rec.elem_ctr + mid, bad);
        if (pm == NONE32) { bad = true; break; }   // (every value of a record is an element of this object)
        if (pm == p) found = true;
        if (pm < p) a = mid + 1; else e = mid;
      }
      position = rec.index + a;
      if (found) {
        status = AM355_POS_VISIBLE;
        if (rec_is_counter(rec)) status |= AM355_POS_COUNTER;
      }
    }
  }
  if (bad) {
    atomicOr(&words[PW_FLAGS], (uint32_t)PF_RANGE);
    status = AM355_POS_UNKNOWN; position = 0;
  }
  am355_elem_pos* out = pinned_or_spill(pinned, spill, i);
  out->position = position;
  out->status = status;
}

}  // namespace am355

namespace {

int text_position_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const am355_elem_id* ids, uint32_t n, const am355_elem_pos** out,
                       uint64_t* length) {
  if (!c) return AM355_E_ARG;
  if (!out || !length || (!obj_actor && actor_len) || (n && !ids)) return fail(c, AM355_E_ARG, "am355_text_position: null argument");
  *out = nullptr; *length = 0;
  TextObject o;   // (on the state of a document's rebuilt changes, whose rows and list order are searched)
  { int orc = text_open(c, "am355_text_position", obj_ctr, obj_actor, actor_len, TO_CHANGE_STATE, &c->n_position_launches, o); if (orc) return orc; }
  hipStream_t st = c->stream;
  const uint32_t R = o.recs.R, oi = o.index, NL = c->counts.n_list_ins;
  MergeBufs& b = c->mb;
  if (b.n_ops != c->n_ops || !b.order || !b.kind || !b.spans) return fail(c, AM355_E_DEVICE, "internal: the op rows of the state are not on the device");
  if (!c->h_pos_out.ensure(((size_t)(n ? n : 1)) * sizeof(am355_elem_pos))) return fail(c, AM355_E_NOMEM, "host allocation failed (position)");
  *out = c->h_pos_out.as<am355_elem_pos>();
  if (R == 0 && n == 0) { c->n_position_served++; return AM355_OK; }   // (an empty Text, nothing asked: nothing to launch)

  // ---- positions: pos_of[row] of the stored order, rebuilt when no in-place merge left it current ----
  if (!c->pos_valid) {
    const size_t cap_rows = std::max<size_t>(b.row_stride, (size_t)c->n_ops + 1);
    if (!c->d_pos.ensure_keep(4 * cap_rows, 0)) return fail(c, AM355_E_NOMEM, "device allocation failed (position)");
    resorder_positions(b, NL, c->d_pos.as<uint32_t>(), st);
    if (NL) c->n_position_launches++;
    c->pos_valid = true;   // (d_pos describes b.order: what the next in-place merge would have built itself)
  }
  if (c->d_pos.cap < 4 * (size_t)c->n_ops) return fail(c, AM355_E_DEVICE, "internal: the position table is shorter than the rows");

  const uint32_t spill_max = n > LOCATE_PINNED_RUNS ? n - LOCATE_PINNED_RUNS : 0u;
  const size_t b_words = carve_size(PW_WORDS, 4), b_rec = carve_size(R, 4), b_ids = carve_size(spill_max ? n : 0, sizeof(am355_elem_id)),
               b_spill = carve_size(spill_max, sizeof(am355_elem_pos));
  if (!c->d_posq.ensure(b_words + b_rec + b_ids + b_spill + 256) || !c->h_pos_ids.ensure(((size_t)(n ? n : 1)) * sizeof(am355_elem_id)))
    return fail(c, AM355_E_NOMEM, "allocation failed (position)");
  uint8_t* dp = c->d_posq.as<uint8_t>();
  uint32_t* dw = (uint32_t*)dp;
  uint32_t* d_rec = (uint32_t*)(dp + b_words);
  am355_elem_id* d_ids = (am355_elem_id*)(dp + b_words + b_rec);
  am355_elem_pos* d_spill = (am355_elem_pos*)(dp + b_words + b_rec + b_ids);
  const PosQuery q{o.recs, c->d_pos.as<uint32_t>(), NL, (uint32_t)obj_ctr, o.actor_rank};
  HIPCHK(c, hipMemsetAsync(dw, 0, PW_WORDS * 4, st));
  if (R) {
    AM355_LAUNCH_INDEPENDENT(kp_heads, dim3((R + BLOCK - 1) / BLOCK), dim3(BLOCK), st, b, q, d_rec, dw);
    c->n_position_launches++;
  }
  if (n) {
    // the queries: up to the pinned bound the kernel reads them where the host put them; more go up in one copy
    const am355_elem_id* src = c->h_pos_ids.as<am355_elem_id>();
    memcpy(c->h_pos_ids.p, ids, (size_t)n * sizeof(am355_elem_id));
    if (spill_max) {
      HIPCHK(c, hipMemcpyAsync(d_ids, c->h_pos_ids.p, (size_t)n * sizeof(am355_elem_id), hipMemcpyHostToDevice, st));
      src = d_ids;
    }
    AM355_LAUNCH_INDEPENDENT(kp_resolve, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), st, b, q, (const uint32_t*)d_rec, src, n, dw, c->h_pos_out.as<am355_elem_pos>(), d_spill);
    c->n_position_launches++;
  }
  c->n_position_launches++;
  // the one wait of the call: flag word and length; the results behind the pinned bound follow in one copy
  HIPCHK(c, c->text_sig.fetch(dw, PW_WORDS, 0, st));
  const uint32_t* hw = c->text_sig.words();
  const uint32_t pf = hw[PW_FLAGS];
  { int prc = text_premise_error(c, TC_POSITION, pf, oi); if (prc) return prc; }
  if (pf & PF_RANGE) return fail(c, AM355_E_DEVICE, "internal: a row or a position of object %u lies outside the tables", oi);
  { int src = spill_down(c, c->h_pos_out.as<am355_elem_pos>(), (const am355_elem_pos*)d_spill, n); if (src) return src; }
  *length = R ? hw[PW_LENGTH] : 0u;
  c->n_position_served++;
  return AM355_OK;
}

}  // namespace

extern "C" int am355_text_position(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const am355_elem_id* ids, uint32_t n,
                                   const am355_elem_pos** out, uint64_t* length) {
  return guarded(c, [&]() { return text_position_impl(c, obj_ctr, obj_actor, actor_len, ids, n, out, length); });
}
extern "C" int am355_rank_of_actor(const am355_ctx* c, const uint8_t* bytes, size_t len, uint32_t* rank) {
  if (!c || !rank || !bytes) return AM355_E_ARG;
  if (!c->replayed) return AM355_E_STATE;
  if (!len) return AM355_E_ARG;   // (no actor has an empty id)
  return actor_rank_of(c, bytes, len, rank) ? AM355_OK : AM355_E_ARG;
}
extern "C" int am355_text_position_calls(const am355_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_position_served;
  out[1] = c->n_position_launches;
  return AM355_OK;
}
extern "C" int am355_text_position_limits(uint32_t out[2]) {
  if (!out) return AM355_E_ARG;
  out[0] = BLOCK; out[1] = LOCATE_PINNED_RUNS;
  return AM355_OK;
}
