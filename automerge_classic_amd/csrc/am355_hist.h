// History reconstruction after Backend.load on the device: see am355_hist.hip.
#pragma once
#include "am355_encode.h"
#include "am355_internal.h"
#include "../../include/am355.h"

namespace am355 {

enum : uint32_t { HF_INVALID = 1u, HF_UNSUPPORTED = 2u };  // HistBufs.flags: what the reference does with this document (throws / served by the JS path)
constexpr int HIST_NCOL = 12;  // change columns in id order: objActor objCtr keyActor keyCtr keyStr insert action valLen valRaw predNum predActor predCtr

// Device memory of the reconstruction. N = document rows, P = succ entries, NC = changes, NA = actors, W = 32-bit words of the id
// bitmaps (one bit per (actor, counter) up to the actor's last maxOp). Every id the document mentions -- row ids and ids in succ lists --
// gets a SLOT: ids numbered per actor in counter order = the order of ops inside a change and of changes inside an actor. M <= N + P.
struct HistBufs {
  uint32_t N, P, NC, NA, W, AW;    // AW = words of a change's actor bitmap
  uint32_t* flags;                 // [4]: HF_* | -- | M (slots) | total preds
  // uploaded by the host
  uint32_t *word_base, *act_max;   // [NA + 1], [NA]
  uint32_t *chg_actor, *chg_prev_max, *chg_max;   // [NC]
  uint32_t *sorted_base, *sorted_chg;             // [NCs] the changes that own slots, ascending by first slot (second upload)
  // ids -> slots
  uint32_t *all_bits, *row_bits, *word_cnt, *word_rank;   // [W + 1]
  uint32_t *slot_row, *slot_ref;   // [M]: row that carries the id | first row that lists it in its succ list (NONE32: none)
  uint32_t *pred_cnt, *pred_first, *pred_cur;    // [M + 1]
  uint32_t* pred_row;              // [P]: rows overwritten by the op in the slot (the inverse of the succ lists), ascending by id per slot
  // changes -> slot ranges
  uint32_t *chg_base, *chg_nops;   // [NC]
  uint32_t* abits;                 // [NC x AW] actors a change mentions
  // the changes' op columns, by slot (seg: first slot of the slot's change) and by pred entry (pseg)
  uint32_t *seg, *chg_of;          // [M]
  uint32_t *v_obj_actor, *v_obj_ctr, *v_key_actor, *v_key_ctr, *v_key_off, *v_key_len, *v_action, *v_val_tl, *v_val_off, *v_pred_num;   // [M]
  uint8_t* v_insert;               // [M]
  uint32_t *p_actor, *p_ctr, *pseg;   // [P]
  uint32_t *seg_base, *pseg_base;  // [NC + 1] first slot / first pred entry of every change (document order of changes)
  // encoder work + output
  EncWork enc;
  uint32_t* deltas;                // [max(M, P) + 2]
  uint8_t* nullmask;               // [max(M, P) + 2]
  uint8_t* col_out[HIST_NCOL];     // encoded bytes of a column, all changes back to back
  size_t col_cap[HIST_NCOL];
  uint32_t* col_off;               // [HIST_NCOL][2 x (NC + 1)]: begin / end of change k in column q at [q][2k], [q][2k + 1]
  uint32_t* col_len;               // [HIST_NCOL] total bytes
  void* scan_ws;
};
size_t hist_bytes(uint32_t N, uint32_t P, uint32_t NC, uint32_t NA, uint32_t W, size_t key_bytes, size_t val_bytes);
void hist_bind(HistBufs& h, void* block, uint32_t N, uint32_t P, uint32_t NC, uint32_t NA, uint32_t W, size_t key_bytes, size_t val_bytes);

// Stage 1 (enqueued on st): id bitmaps, slots, preds by slot, slot range of every change. Afterwards the host reads h.flags,
// h.chg_base, h.chg_nops (it needs the changes that own slots in slot order for stage 2, and the op counts for the headers).
void hist_stage1(const OpCols& rows, HistBufs& h, hipStream_t st);
// Stage 2: actor tables, the op columns of every change (values by slot), the twelve column encodes segmented by change.
// n_sorted: entries of h.sorted_base / h.sorted_chg. Afterwards h.col_out / h.col_off / h.col_len / h.abits / h.flags are complete.
void hist_stage2(const OpCols& rows, const uint8_t* arena, size_t arena_len, HistBufs& h, uint32_t n_sorted, uint32_t M, hipStream_t st);

// A local change REQUEST (include/am355.h am355_local_change) turned into the value arrays the same twelve encodes read. The request's
// arrays are uploaded as one block (`up`, the layout local_bind gives both the pinned and the device copy); HistBufs is bound with
// N = rows, P = pred_rows, NC = 1 and its v_* / p_* / col_* members are used as by hist_stage2, with one segment.
struct LocalBufs {
  uint32_t n_ops, n_values, n_preds, n_actors, rows, pred_rows, str_len, val_cap, start_op;
  // uploaded
  am355_local_op* ops;          // [n_ops]
  am355_local_value* values;    // [n_values]
  am355_local_pred* preds;      // [n_preds]
  uint32_t* rank;               // [n_actors]
  uint32_t *multi, *pcnt;       // [n_ops + 1] rows / pred entries an op expands to (last: 0)
  uint8_t* arena;               // [str_len] keys and UTF-8 values | [val_cap] the value bytes of the rows, written by kl_values
  size_t up_bytes;              // the block up to and including the strings: what the host fills and uploads
  // device only
  uint32_t *row_base, *pred_base;   // [n_ops + 1]
  uint32_t *vidx, *vlen, *voff;     // [rows + 1] value record of a row (NONE32: none) | its bytes | their offset behind str_len
  void* scan_ws;
};
size_t local_bytes(uint32_t n_ops, uint32_t n_values, uint32_t n_preds, uint32_t n_actors, uint32_t rows, uint32_t str_len, uint32_t val_cap);
// carves `block` (device or pinned: the same offsets); only the uploaded members are valid for a pinned block of up_bytes
void local_bind(LocalBufs& L, void* block, uint32_t n_ops, uint32_t n_values, uint32_t n_preds, uint32_t n_actors, uint32_t rows, uint32_t pred_rows, uint32_t str_len,
                uint32_t val_cap, uint32_t start_op);
// scans, kl_expand, kl_values, the twelve encodes (enqueued on st). Afterwards h.flags / h.col_len / h.col_out are complete.
void local_expand_encode(const LocalBufs& L, HistBufs& h, hipStream_t st);

// A SMALL local change (am355_set_local_small): ONE workgroup does all of the above in LDS -- the scans, the expansion, the value bytes,
// the twelve encodes -- and writes the columns, their lengths and the flag word straight into pinned host memory (kl_small). The limits
// are what its LDS carve holds; a request inside all four is built that way, every other one by local_expand_encode.
constexpr uint32_t LOCAL_SMALL_ROWS = 512;     // rows of the expanded change
constexpr uint32_t LOCAL_SMALL_PREDS = 512;    // pred entries of the expanded change
constexpr uint32_t LOCAL_SMALL_OPS = 256;      // ops of the request
constexpr uint32_t LOCAL_SMALL_BYTES = 4096;   // key bytes (once per row) + value bytes (8 per number, a string's length)
// worst case of the twelve columns together: nine numeric columns and the boolean one by enc_numbers_bound (seven and the boolean over
// rows, two over pred entries), keyStr = a numeric column + the key bytes, valRaw = the value bytes
constexpr size_t LOCAL_SMALL_OUT_BYTES = 9 * (10 * (size_t)LOCAL_SMALL_ROWS + 16) + 2 * (10 * (size_t)LOCAL_SMALL_PREDS + 16) + 2 * ((size_t)LOCAL_SMALL_BYTES + 16);
constexpr size_t LOCAL_SMALL_HEAD = 256;       // in front of the column bytes: flags[4] | col_len[HIST_NCOL]
inline size_t local_small_host_bytes() { return LOCAL_SMALL_HEAD + LOCAL_SMALL_OUT_BYTES; }
inline bool local_small_fits(uint32_t n_ops, uint64_t rows, uint64_t pred_rows, uint64_t key_val_bytes) {
  return n_ops <= LOCAL_SMALL_OPS && rows <= LOCAL_SMALL_ROWS && pred_rows <= LOCAL_SMALL_PREDS && key_val_bytes <= LOCAL_SMALL_BYTES;
}
// One launch on st. `L`: the device block the request was uploaded into (only its uploaded members are read). `host_out`: pinned,
// local_small_host_bytes(): flags[0] != 0 when the kernel refused (a count beyond its carve); else col_len and the columns back to back
// from LOCAL_SMALL_HEAD on, in id order.
void local_small_encode(const LocalBufs& L, uint8_t* host_out, hipStream_t st);

}  // namespace am355
