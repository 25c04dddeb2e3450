// History reconstruction after Backend.load, device part.
//
// Reference: backend/new.js:1887-1912 computeHashGraph -> backend/columnar.js:1040-1047 decodeDocument, :876-943 groupChangeOps
// (ops -> changes by (actor, maxOp); `del` ops rebuilt from succ entries; preds = inverse of succ), :945-981 decodeDocumentChanges,
// :710-739 encodeChange, :370-444 encodeOps, :122-170 parseAllOpIds (change-local actor table: author first, the others sorted).
//
// A saved document holds the merged op rows, not its changes. The rows are in HBM after the load (am355_bigcol.hip); here:
//   1. ids -> slots: one bit per (actor, counter) that a row carries or a succ list names; popcount + prefix sum ranks the bits, which
//      numbers the ids per actor in counter order -- the order of ops inside a change and of changes inside an actor. An id no row
//      carries is a deletion: groupChangeOps rebuilds a `del` op for it from the first row that lists it (kh_mark, kh_popc, kh_slots);
//   2. preds = the inverse of the succ lists: counts per slot, prefix sum, fill, order by (counter, actor) (kh_pred_fill, kh_pred_sort);
//   3. a change owns the ids in (maxOp of its actor's previous change, maxOp]: its slot range by two rank queries (kh_changes);
//   4. the actors a change mentions (bitmap per change; the change-local index of an actor = its rank among them, author first) and
//      the twelve op columns of ALL changes as arrays by slot (kh_refs, kh_rows), validated as the reference's decode / re-encode
//      round trip would;
//   5. the column encoders of Backend.save (am355_encode.hip), segmented by change: one pass per column encodes that column of every
//      change (hist_stage2).
// The host (am355_history.cpp) reads the change metadata columns (a few thousand values), writes the headers, copies the column
// pieces into place and chains the hashes: a change's header holds the hashes of its dependencies, so SHA-256 runs level by level
// of the dependency graph, one dependent 64-byte block after the other per change -- 16 MB/s for a lane of this device against
// 2 GB/s for a host core with SHA extensions; the chain stays on the host threads.
#include "am355_hist.h"
#include "am355_prims.h"
#include "am355_scan.h"

namespace am355 {

static inline dim3 grid_for(uint32_t n) { return dim3((n + BLOCK - 1) / BLOCK); }
static size_t al256(size_t b) { return carve_round(b); }

static size_t hist_col_cap(int k, uint32_t M, uint32_t P, size_t key_bytes, size_t val_bytes) {
  // keyStr: headers + length prefixes + the key bytes. `key_bytes` is the caller's estimate -- the document's own key column holds a
  // repeated key once, the changes hold it once per change, so the rebuilt columns can be far longer than it; the encoder never
  // writes past this bound and reports the size it needs, with which the caller binds again (am355_doc_changes)
  if (k == 4) return enc_numbers_bound(M) + key_bytes + 16;
  if (k == 8) return val_bytes + 16;                          // valRaw
  return enc_numbers_bound(k >= 10 ? P : M);
}

size_t hist_bytes(uint32_t N, uint32_t P, uint32_t NC, uint32_t NA, uint32_t W, size_t key_bytes, size_t val_bytes) {
  const size_t M = (size_t)N + P + 1, PP = (size_t)P + 1, C = (size_t)NC + 1, AW = ((size_t)NA + 31) / 32, big = (M > PP ? M : PP) + 2;
  size_t b = al256(16) + al256(4 * ((size_t)NA + 1)) + al256(4 * (size_t)NA + 4) + 5 * al256(4 * C) + 4 * al256(4 * ((size_t)W + 2));
  b += 2 * al256(4 * M) + 3 * al256(4 * (M + 1)) + al256(4 * PP) + 2 * al256(4 * C) + al256(4 * C * AW);
  b += 12 * al256(4 * M) + al256(M) + 3 * al256(4 * PP) + 2 * al256(4 * (C + 1));
  b += al256(enc_work_bytes((uint32_t)big)) + al256(4 * big) + al256(big) + al256(4 * HIST_NCOL * 2 * (C + 1)) + al256(4 * HIST_NCOL);
  for (int k = 0; k < HIST_NCOL; k++) b += al256(hist_col_cap(k, (uint32_t)M, (uint32_t)PP, key_bytes, val_bytes));
  b += al256(scan_workspace_bytes((uint32_t)std::max<size_t>(big, (size_t)W + 2)));
  return b + 4096;
}

void hist_bind(HistBufs& h, void* block, uint32_t N, uint32_t P, uint32_t NC, uint32_t NA, uint32_t W, size_t key_bytes, size_t val_bytes) {
  canary_scope("history reconstruction (hist_bind)");
  canary_forget(block, hist_bytes(N, P, NC, NA, W, key_bytes, val_bytes));
  const size_t M = (size_t)N + P + 1, PP = (size_t)P + 1, C = (size_t)NC + 1, AW = ((size_t)NA + 31) / 32, big = (M > PP ? M : PP) + 2;
  uint8_t* p = (uint8_t*)block;
  auto take = [&](size_t bytes) { void* r = p; canary_note(p, bytes); p += al256(bytes); return r; };
  h.N = N; h.P = P; h.NC = NC; h.NA = NA; h.W = W; h.AW = (uint32_t)AW;
  h.flags = (uint32_t*)take(16);
  h.word_base = (uint32_t*)take(4 * ((size_t)NA + 1)); h.act_max = (uint32_t*)take(4 * (size_t)NA + 4);
  h.chg_actor = (uint32_t*)take(4 * C); h.chg_prev_max = (uint32_t*)take(4 * C); h.chg_max = (uint32_t*)take(4 * C);
  h.sorted_base = (uint32_t*)take(4 * C); h.sorted_chg = (uint32_t*)take(4 * C);
  h.all_bits = (uint32_t*)take(4 * ((size_t)W + 2)); h.row_bits = (uint32_t*)take(4 * ((size_t)W + 2));
  h.word_cnt = (uint32_t*)take(4 * ((size_t)W + 2)); h.word_rank = (uint32_t*)take(4 * ((size_t)W + 2));
  h.slot_row = (uint32_t*)take(4 * M); h.slot_ref = (uint32_t*)take(4 * M);
  h.pred_cnt = (uint32_t*)take(4 * (M + 1)); h.pred_first = (uint32_t*)take(4 * (M + 1)); h.pred_cur = (uint32_t*)take(4 * (M + 1));
  h.pred_row = (uint32_t*)take(4 * PP);
  h.chg_base = (uint32_t*)take(4 * C); h.chg_nops = (uint32_t*)take(4 * C);
  h.abits = (uint32_t*)take(4 * C * AW);
  h.seg = (uint32_t*)take(4 * M); h.chg_of = (uint32_t*)take(4 * M);
  uint32_t** vs[] = {&h.v_obj_actor, &h.v_obj_ctr, &h.v_key_actor, &h.v_key_ctr, &h.v_key_off, &h.v_key_len, &h.v_action, &h.v_val_tl, &h.v_val_off, &h.v_pred_num};
  for (uint32_t** v : vs) *v = (uint32_t*)take(4 * M);
  h.v_insert = (uint8_t*)take(M);
  h.p_actor = (uint32_t*)take(4 * PP); h.p_ctr = (uint32_t*)take(4 * PP); h.pseg = (uint32_t*)take(4 * PP);
  h.seg_base = (uint32_t*)take(4 * (C + 1)); h.pseg_base = (uint32_t*)take(4 * (C + 1));
  {
    void* w = take(enc_work_bytes((uint32_t)big));
    enc_carve(h.enc, w, (uint32_t)big);
    canary_scope("history reconstruction (hist_bind, behind the encoder work)");
  }
  h.deltas = (uint32_t*)take(4 * big);
  h.nullmask = (uint8_t*)take(big);
  h.col_off = (uint32_t*)take(4 * HIST_NCOL * 2 * (C + 1));
  h.col_len = (uint32_t*)take(4 * HIST_NCOL);
  for (int k = 0; k < HIST_NCOL; k++) {
    h.col_cap[k] = hist_col_cap(k, (uint32_t)M, (uint32_t)PP, key_bytes, val_bytes);
    h.col_out[k] = (uint8_t*)take(h.col_cap[k]);
  }
  h.scan_ws = take(scan_workspace_bytes((uint32_t)std::max<size_t>(big, (size_t)W + 2)));
}

// ---------------------------------------------------------------------------------------------------------
// ids -> slots
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool id_in_range(const HistBufs& h, uint32_t a, uint32_t ctr) { return a < h.NA && ctr != 0 && ctr <= h.act_max[a]; }

__global__ __launch_bounds__(BLOCK) void kh_mark(OpCols rows, HistBufs h) {
  const uint32_t i = gtid();
  if (i < h.N) {
    const uint32_t a = rows.id_actor[i], ctr = rows.id_ctr[i];
    if (!id_in_range(h, a, ctr)) atomicOr(&h.flags[0], (uint32_t)HF_INVALID);   // operation id outside of the range its actor's changes allow
    else {
      const uint32_t w = h.word_base[a] + ctr / 32, bit = 1u << (ctr % 32);
      if (atomicOr(&h.row_bits[w], bit) & bit) atomicOr(&h.flags[0], (uint32_t)HF_INVALID);   // two rows carry one operation id
      atomicOr(&h.all_bits[w], bit);
    }
    if ((uint64_t)rows.pred_first[i] + rows.pred_num[i] > h.P) atomicOr(&h.flags[0], (uint32_t)HF_INVALID);  // succ lists exceed the succ columns
  }
  if (i < h.P) {
    const uint32_t a = rows.pred_actor[i], ctr = rows.pred_ctr[i];   // (a document: the succ columns)
    if (!id_in_range(h, a, ctr)) atomicOr(&h.flags[0], (uint32_t)HF_INVALID);
    else atomicOr(&h.all_bits[h.word_base[a] + ctr / 32], 1u << (ctr % 32));
  }
}

__global__ __launch_bounds__(BLOCK) void kh_popc(HistBufs h) {
  const uint32_t w = gtid();
  if (w <= h.W) h.word_cnt[w] = w < h.W ? (uint32_t)__popc(h.all_bits[w]) : 0u;
}

// ids of actor a with a smaller counter, plus the actor's first slot = the slot of (a, ctr) when that id exists
__device__ __forceinline__ uint32_t slot_of(const HistBufs& h, uint32_t a, uint32_t ctr) {
  const uint32_t w = h.word_base[a] + ctr / 32;
  return h.word_rank[w] + (uint32_t)__popc(h.all_bits[w] & ((1u << (ctr % 32)) - 1u));
}

__global__ __launch_bounds__(BLOCK) void kh_slots(OpCols rows, HistBufs h) {
  const uint32_t r = gtid();
  if (r >= h.N) return;
  if (h.flags[0] & HF_INVALID) return;
  h.slot_row[slot_of(h, rows.id_actor[r], rows.id_ctr[r])] = r;
  const uint32_t f = rows.pred_first[r], n = rows.pred_num[r];
  for (uint32_t e = f; e < f + n; e++) {
    const uint32_t s = slot_of(h, rows.pred_actor[e], rows.pred_ctr[e]);
    atomicMin(&h.slot_ref[s], r);
    atomicAdd(&h.pred_cnt[s], 1u);
  }
}

__global__ __launch_bounds__(BLOCK) void kh_pred_fill(OpCols rows, HistBufs h) {
  const uint32_t r = gtid();
  if (r >= h.N) return;
  if (h.flags[0] & HF_INVALID) return;
  const uint32_t f = rows.pred_first[r], n = rows.pred_num[r];
  for (uint32_t e = f; e < f + n; e++) {
    const uint32_t s = slot_of(h, rows.pred_actor[e], rows.pred_ctr[e]);
    h.pred_row[h.pred_first[s] + atomicAdd(&h.pred_cur[s], 1u)] = r;
  }
}

// the preds of an op ascend by (counter, actor) (columnar.js:394-396 sorts them when a change is encoded)
__global__ __launch_bounds__(BLOCK) void kh_pred_sort(OpCols rows, HistBufs h, uint32_t M) {
  const uint32_t s = gtid();
  if (s >= M) return;
  if (h.flags[0] & HF_INVALID) return;
  const uint32_t lo = h.pred_first[s], hi = h.pred_first[s + 1];
  for (uint32_t i = lo + 1; i < hi; i++) {
    const uint32_t r = h.pred_row[i];
    const unsigned long long key = (unsigned long long)rows.id_ctr[r] << 32 | rows.id_actor[r];
    uint32_t j = i;
    for (; j > lo; j--) {
      const uint32_t q = h.pred_row[j - 1];
      if (((unsigned long long)rows.id_ctr[q] << 32 | rows.id_actor[q]) <= key) break;
      h.pred_row[j] = q;
    }
    h.pred_row[j] = r;
  }
}

__global__ __launch_bounds__(BLOCK) void kh_changes(HistBufs h) {
  const uint32_t k = gtid();
  if (k >= h.NC) return;
  if (h.flags[0] & HF_INVALID) { h.chg_base[k] = 0; h.chg_nops[k] = 0; return; }
  const uint32_t a = h.chg_actor[k], mx = h.chg_max[k], prev = h.chg_prev_max[k];
  const uint32_t base = slot_of(h, a, prev + 1), n = slot_of(h, a, mx + 1) - base;
  h.chg_base[k] = base;
  h.chg_nops[k] = n;
  bool bad = n > mx;   // more operations than maxOp allows
  // ids must be startOp .. maxOp without a gap (columnar.js:935-939)
  if (!bad && n && slot_of(h, a, mx - n + 1) != base) bad = true;
  if (bad) atomicOr(&h.flags[0], (uint32_t)HF_INVALID);
  if (k == 0) { h.flags[2] = h.word_rank[h.W]; h.flags[3] = h.pred_first[h.word_rank[h.W]]; }
}

void hist_stage1(const OpCols& rows, HistBufs& h, hipStream_t st) {
  const uint32_t Mcap = h.N + h.P + 1;
  (void)hipMemsetAsync(h.flags, 0, 16, st);
  (void)hipMemsetAsync(h.all_bits, 0, 4 * ((size_t)h.W + 2), st);
  (void)hipMemsetAsync(h.row_bits, 0, 4 * ((size_t)h.W + 2), st);
  (void)hipMemsetAsync(h.slot_row, 0xff, 4 * (size_t)Mcap, st);
  (void)hipMemsetAsync(h.slot_ref, 0xff, 4 * (size_t)Mcap, st);
  (void)hipMemsetAsync(h.pred_cnt, 0, 4 * ((size_t)Mcap + 1), st);
  (void)hipMemsetAsync(h.pred_cur, 0, 4 * ((size_t)Mcap + 1), st);
  const uint32_t np = h.N > h.P ? h.N : h.P;
  if (np) AM355_LAUNCH_INDEPENDENT(kh_mark, grid_for(np), dim3(BLOCK), st, rows, h);
  AM355_LAUNCH_INDEPENDENT(kh_popc, grid_for(h.W + 1), dim3(BLOCK), st, h);
  exclusive_scan_u32(h.word_cnt, h.word_rank, h.W + 1, nullptr, h.scan_ws, st);
  if (h.N) AM355_LAUNCH_INDEPENDENT(kh_slots, grid_for(h.N), dim3(BLOCK), st, rows, h);
  exclusive_scan_u32(h.pred_cnt, h.pred_first, Mcap + 1, nullptr, h.scan_ws, st);
  if (h.N) AM355_LAUNCH_INDEPENDENT(kh_pred_fill, grid_for(h.N), dim3(BLOCK), st, rows, h);
  AM355_LAUNCH_INDEPENDENT(kh_pred_sort, grid_for(Mcap), dim3(BLOCK), st, rows, h, Mcap);
  if (h.NC) AM355_LAUNCH_INDEPENDENT(kh_changes, grid_for(h.NC), dim3(BLOCK), st, h);
}

// ---------------------------------------------------------------------------------------------------------
// the changes' op columns
// ---------------------------------------------------------------------------------------------------------
// change that owns slot s: the last entry of sorted_base <= s (only changes that own slots are listed)
__device__ __forceinline__ uint32_t change_of_slot(const HistBufs& h, uint32_t n_sorted, uint32_t s) {
  uint32_t lo = 0, hi = n_sorted;
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (h.sorted_base[mid] <= s) lo = mid; else hi = mid;
  }
  return h.sorted_chg[lo];
}

__device__ __forceinline__ void touch(const HistBufs& h, uint32_t k, uint32_t a) { atomicOr(&h.abits[(size_t)k * h.AW + a / 32], 1u << (a % 32)); }

// index of actor a in the actor table of change k: the author first, the others in id order = rank order (columnar.js:154-157)
__device__ __forceinline__ uint32_t local_actor(const HistBufs& h, uint32_t k, uint32_t a) {
  const uint32_t author = h.chg_actor[k];
  if (a == author) return 0;
  const uint32_t* bits = h.abits + (size_t)k * h.AW;
  uint32_t n = 0;
  for (uint32_t w = 0; w < a / 32; w++) n += (uint32_t)__popc(bits[w]);
  n += (uint32_t)__popc(bits[a / 32] & ((1u << (a % 32)) - 1u));
  return author < a ? n : n + 1;   // (the author's own bit is set as well)
}

// pass 1 over the slots: which change, which witness row, which actors the change mentions
__global__ __launch_bounds__(BLOCK) void kh_refs(OpCols rows, HistBufs h, uint32_t n_sorted, uint32_t M) {
  const uint32_t s = gtid();
  if (s >= M) return;
  const uint32_t k = change_of_slot(h, n_sorted, s);
  h.chg_of[s] = k;
  h.seg[s] = h.chg_base[k];
  const uint32_t r = h.slot_row[s];
  const uint32_t q = r != NONE32 ? r : h.slot_ref[s];
  if (q == NONE32) { atomicOr(&h.flags[0], (uint32_t)HF_INVALID); return; }   // operation without a row
  touch(h, k, h.chg_actor[k]);
  if (rows.obj_actor[q] != NONE32) {
    if (rows.obj_actor[q] >= h.NA) { atomicOr(&h.flags[0], (uint32_t)HF_INVALID); return; }
    touch(h, k, rows.obj_actor[q]);
  }
  if (rows.key_len[q] == NONE32) {
    if (r == NONE32 && rows.insert[q]) touch(h, k, rows.id_actor[q]);
    else if (rows.key_ctr[q] != 0 && rows.key_ctr[q] != NONE32) {
      if (rows.key_actor[q] >= h.NA) { atomicOr(&h.flags[0], (uint32_t)HF_INVALID); return; }
      touch(h, k, rows.key_actor[q]);
    }
  }
  for (uint32_t e = h.pred_first[s]; e < h.pred_first[s + 1]; e++) touch(h, k, rows.id_actor[h.pred_row[e]]);
}

// valid UTF-8 that TextDecoder -> TextEncoder reproduces (a leading U+FEFF is dropped by the decoder, encoding.js:9-17)
__device__ bool hist_valid_utf8(const uint8_t* s, uint32_t n) {
  if (n >= 3 && s[0] == 0xef && s[1] == 0xbb && s[2] == 0xbf) return false;
  uint32_t i = 0;
  while (i < n) {
    const uint8_t c = s[i];
    if (c < 0x80) { i++; continue; }
    uint32_t extra, cp;
    if ((c & 0xe0) == 0xc0) { extra = 1; cp = c & 0x1f; }
    else if ((c & 0xf0) == 0xe0) { extra = 2; cp = c & 0x0f; }
    else if ((c & 0xf8) == 0xf0) { extra = 3; cp = c & 0x07; }
    else return false;
    if (i + extra >= n) return false;
    for (uint32_t j = 1; j <= extra; j++) {
      if ((s[i + j] & 0xc0) != 0x80) return false;
      cp = cp << 6 | (s[i + j] & 0x3f);
    }
    if ((extra == 1 && cp < 0x80) || (extra == 2 && cp < 0x800) || (extra == 3 && (cp < 0x10000 || cp > 0x10ffff)) || (cp >= 0xd800 && cp <= 0xdfff)) return false;
    i += extra + 1;
  }
  return true;
}

// A value the reference's decodeValue -> encodeValue round trip (columnar.js:259-329) reproduces byte for byte? 0 yes; HF_INVALID: the
// reference throws on it; HF_UNSUPPORTED: the reference writes something else (numbers not in minimal form, byte arrays -- encodeValue
// writes the whole underlying buffer of a decoded byte array --, unknown type tags)
__device__ uint32_t hist_value_round_trips(uint32_t tl, const uint8_t* b) {
  const uint32_t tag = tl & 15, len = tl >> 4;
  switch (tag) {
    case 0: case 1: case 2: return len ? (uint32_t)HF_UNSUPPORTED : 0u;
    case 3: case 4: case 8: case 9: {
      // one LEB128 number filling the value exactly, inside +-2^53, in its shortest form
      if (len == 0 || len > 10) return HF_INVALID;
      unsigned long long v = 0;
      uint32_t shift = 0, i = 0;
      for (; i < len; i++) {
        const uint8_t c = b[i];
        if (shift < 64) v |= (unsigned long long)(c & 0x7f) << shift;
        shift += 7;
        if (!(c & 0x80)) break;
      }
      if (i + 1 != len) return HF_INVALID;   // ends early or runs past the value
      if (tag == 3) {
        if (shift > 63 || v >= (1ull << 53)) return HF_INVALID;
        uint32_t need = 1;
        for (unsigned long long x = v; x >= 0x80; x >>= 7) need++;
        return need == len ? 0u : (uint32_t)HF_UNSUPPORTED;
      }
      long long sv = (long long)v;
      if ((b[len - 1] & 0x40) && shift < 64) sv = (long long)(v | (~0ull << shift));
      if (shift > 63 + 7 || sv >= (1ll << 53) || sv <= -(1ll << 53)) return HF_INVALID;
      uint32_t need = 1;
      for (long long x = sv;; need++) {
        const uint8_t c = (uint8_t)(x & 0x7f);
        x >>= 7;
        if ((x == 0 && !(c & 0x40)) || (x == -1 && (c & 0x40))) break;
      }
      return need == len ? 0u : (uint32_t)HF_UNSUPPORTED;
    }
    case 5: return len == 8 ? 0u : (uint32_t)HF_INVALID;
    case 6: return hist_valid_utf8(b, len) ? 0u : (uint32_t)HF_UNSUPPORTED;
    default: return HF_UNSUPPORTED;
  }
}

// pass 2 over the slots: the op of the slot as the values of its change's columns (encodeOps, columnar.js:370-444)
__global__ __launch_bounds__(BLOCK) void kh_rows(OpCols rows, const uint8_t* __restrict__ arena, unsigned long long arena_len, HistBufs h, uint32_t M) {
  const uint32_t s = gtid();
  if (s >= M) return;
  if (h.flags[0] & HF_INVALID) return;
  const uint32_t k = h.chg_of[s], r = h.slot_row[s];
  const bool del = r == NONE32;
  const uint32_t q = del ? h.slot_ref[s] : r;
  uint32_t err = 0;
  uint32_t oa = NONE32, oc = NONE32, ka = NONE32, kc = NONE32, koff = 0, klen = NONE32;
  if (rows.obj_actor[q] != NONE32) { oa = local_actor(h, k, rows.obj_actor[q]); oc = rows.obj_ctr[q]; }
  if (rows.key_len[q] != NONE32) {
    klen = rows.key_len[q]; koff = rows.key_off[q];
    if (klen == 0) err |= HF_UNSUPPORTED;                                           // empty map key
    else if ((unsigned long long)koff + klen > arena_len) err |= HF_INVALID;          // key outside the arena
    else if (!hist_valid_utf8(arena + koff, klen)) err |= HF_UNSUPPORTED;             // key is not valid UTF-8
  } else if (del && rows.insert[q]) {   // deleting the element the witness row inserted
    ka = local_actor(h, k, rows.id_actor[q]); kc = rows.id_ctr[q];
  } else if (rows.key_ctr[q] == 0) {
    if (del || !rows.insert[q]) err |= HF_INVALID;                                  // operation on _head that is not an insertion
    kc = 0;
  } else if (rows.key_ctr[q] != NONE32) {
    ka = local_actor(h, k, rows.key_actor[q]); kc = rows.key_ctr[q];
  } else err |= HF_INVALID;                                                          // operation without a key
  const uint32_t act = del ? 3u : rows.action[q];
  if (!del && act == 3) err |= HF_INVALID;                                           // a document holds no del operations
  if (act >= 7) err |= HF_UNSUPPORTED;                                               // link or unknown action
  uint32_t tl = 0, voff = 0;
  if (!del && (act == 1 || act == 5)) {
    tl = rows.val_tl[q]; voff = rows.val_off[q];
    const uint32_t len = tl >> 4;
    if (len && (unsigned long long)voff + len > arena_len) err |= HF_INVALID;         // value outside the arena
    else err |= hist_value_round_trips(tl, arena + voff);
  }
  h.v_obj_actor[s] = oa; h.v_obj_ctr[s] = oc; h.v_key_actor[s] = ka; h.v_key_ctr[s] = kc; h.v_key_off[s] = koff; h.v_key_len[s] = klen;
  h.v_insert[s] = del ? 0 : rows.insert[q];
  h.v_action[s] = act; h.v_val_tl[s] = tl; h.v_val_off[s] = voff;
  const uint32_t pf = h.pred_first[s], pn = h.pred_first[s + 1] - pf;
  h.v_pred_num[s] = pn;
  const uint32_t pbase = h.pred_first[h.chg_base[k]];
  for (uint32_t e = pf; e < pf + pn; e++) {
    const uint32_t pr = h.pred_row[e];
    h.p_actor[e] = local_actor(h, k, rows.id_actor[pr]);
    h.p_ctr[e] = rows.id_ctr[pr];
    h.pseg[e] = pbase;
  }
  if (err) atomicOr(&h.flags[0], err);
}

// first slot / first pred entry of every change in DOCUMENT order of the changes (a change without ops: an empty range)
__global__ __launch_bounds__(BLOCK) void kh_seg_bases(HistBufs h, uint32_t M) {
  const uint32_t k = gtid();
  if (k > h.NC) return;
  if (k == h.NC) { h.seg_base[k] = M; h.pseg_base[k] = h.pred_first[M]; return; }
  // (an empty change sits where the next op of its actor would: an empty stretch wherever it points)
  h.seg_base[k] = h.chg_base[k];
  h.pseg_base[k] = h.pred_first[h.chg_base[k]];
}

// byte range of change k in column c: [col_off[c][2k], col_off[c][2k + 1]) -- changes are not in slot order, so begin and end are
// taken separately from the offsets of the change's first slot and of the slot behind its last
__global__ __launch_bounds__(BLOCK) void kh_col_ranges(HistBufs h, int c, bool by_pred, bool raw, uint32_t n_vals) {
  const uint32_t k = gtid();
  if (k >= h.NC) return;
  const uint32_t b = by_pred ? h.pseg_base[k] : h.seg_base[k];
  const uint32_t n = by_pred ? h.pred_first[h.chg_base[k] + h.chg_nops[k]] - h.pred_first[h.chg_base[k]] : h.chg_nops[k];
  const uint32_t e = b + n;
  uint32_t *out = h.col_off + (size_t)c * 2 * (h.NC + 1);
  if (raw) { out[2 * k] = h.enc.off_ex[b]; out[2 * k + 1] = h.enc.off_ex[e]; }
  else { out[2 * k] = h.enc.off_ex[h.enc.run_ex[b]]; out[2 * k + 1] = h.enc.off_ex[h.enc.run_ex[e < n_vals ? e : n_vals]]; }
}

// The twelve column encodes of change ops given as value arrays by row ([0, M): v_*, segments h.seg) and by pred entry ([0, h.P): p_*,
// segments h.pseg) -- every change a segment. after(column, by_pred, raw, n_vals) runs behind each encode, while h.enc still describes it.
template <class After>
static void hist_encode_columns(const uint8_t* arena, HistBufs& h, uint32_t M, hipStream_t st, After after) {
  enc_rle_numbers(h.v_obj_actor, nullptr, M, false, h.enc, h.col_out[0], h.col_len + 0, st, h.seg); after(0, false, false, M);
  enc_rle_numbers(h.v_obj_ctr, nullptr, M, false, h.enc, h.col_out[1], h.col_len + 1, st, h.seg); after(1, false, false, M);
  enc_rle_numbers(h.v_key_actor, nullptr, M, false, h.enc, h.col_out[2], h.col_len + 2, st, h.seg); after(2, false, false, M);
  enc_delta_prepare(h.v_key_ctr, M, h.deltas, h.nullmask, h.enc, st, h.seg);
  enc_rle_numbers(h.deltas, h.nullmask, M, true, h.enc, h.col_out[3], h.col_len + 3, st, h.seg); after(3, false, false, M);
  enc_rle_strings(arena, h.v_key_off, h.v_key_len, M, h.enc, h.col_out[4], h.col_len + 4, st, h.seg, (uint32_t)std::min<size_t>(h.col_cap[4], 0xffffffffu)); after(4, false, false, M);
  enc_boolean(h.v_insert, M, h.enc, h.col_out[5], h.col_len + 5, st, h.seg); after(5, false, false, M);
  enc_rle_numbers(h.v_action, nullptr, M, false, h.enc, h.col_out[6], h.col_len + 6, st, h.seg); after(6, false, false, M);
  enc_rle_numbers(h.v_val_tl, nullptr, M, false, h.enc, h.col_out[7], h.col_len + 7, st, h.seg); after(7, false, false, M);
  enc_raw_values(arena, h.v_val_off, h.v_val_tl, M, h.enc, h.col_out[8], h.col_len + 8, st); after(8, false, true, M);
  enc_rle_numbers(h.v_pred_num, nullptr, M, false, h.enc, h.col_out[9], h.col_len + 9, st, h.seg); after(9, false, false, M);
  // (the pred columns run over the pred entries: their count sits in flags[3], the host passes it as h.P for this stage)
  if (h.P) {
    enc_rle_numbers(h.p_actor, nullptr, h.P, false, h.enc, h.col_out[10], h.col_len + 10, st, h.pseg); after(10, true, false, h.P);
    enc_delta_prepare(h.p_ctr, h.P, h.deltas, h.nullmask, h.enc, st, h.pseg);
    enc_rle_numbers(h.deltas, h.nullmask, h.P, true, h.enc, h.col_out[11], h.col_len + 11, st, h.pseg); after(11, true, false, h.P);
  }
}

void hist_stage2(const OpCols& rows, const uint8_t* arena, size_t arena_len, HistBufs& h, uint32_t n_sorted, uint32_t M, hipStream_t st) {
  (void)hipMemsetAsync(h.abits, 0, 4 * (size_t)(h.NC + 1) * h.AW, st);
  (void)hipMemsetAsync(h.col_len, 0, 4 * HIST_NCOL, st);
  (void)hipMemsetAsync(h.col_off, 0, 4 * (size_t)HIST_NCOL * 2 * (h.NC + 1), st);
  if (M) {
    AM355_LAUNCH_INDEPENDENT(kh_refs, grid_for(M), dim3(BLOCK), st, rows, h, n_sorted, M);
    AM355_LAUNCH_INDEPENDENT(kh_rows, grid_for(M), dim3(BLOCK), st, rows, arena, (unsigned long long)arena_len, h, M);
  }
  AM355_LAUNCH_INDEPENDENT(kh_seg_bases, grid_for(h.NC + 1), dim3(BLOCK), st, h, M);
  if (!M) return;
  // the twelve columns, every one segmented by change; after each encode the byte range of every change in it
  hist_encode_columns(arena, h, M, st, [&](int c, bool by_pred, bool raw, uint32_t n_vals) {
    AM355_LAUNCH_INDEPENDENT(kh_col_ranges, grid_for(h.NC), dim3(BLOCK), st, h, c, by_pred, raw, n_vals);
  });
}

// ---------------------------------------------------------------------------------------------------------
// a local change request -> the same value arrays (include/am355.h am355_local_change; backend/columnar.js:446-475 expandMultiOps,
// :122-170 parseAllOpIds, :259-292 encodeValue, :394-396 / :423 the pred order)
// ---------------------------------------------------------------------------------------------------------
size_t local_bytes(uint32_t n_ops, uint32_t n_values, uint32_t n_preds, uint32_t n_actors, uint32_t rows, uint32_t str_len, uint32_t val_cap) {
  const size_t O = (size_t)n_ops + 1, R = (size_t)rows + 1;
  return al256(sizeof(am355_local_op) * O) + al256(sizeof(am355_local_value) * ((size_t)n_values + 1)) + al256(sizeof(am355_local_pred) * ((size_t)n_preds + 1)) +
         al256(4 * ((size_t)n_actors + 1)) + 4 * al256(4 * O) + al256((size_t)str_len + val_cap + 16) + 3 * al256(4 * R) + al256(2 * scan_workspace_bytes((uint32_t)std::max(O, R))) + 4096;
}

void local_bind(LocalBufs& L, void* block, uint32_t n_ops, uint32_t n_values, uint32_t n_preds, uint32_t n_actors, uint32_t rows, uint32_t pred_rows, uint32_t str_len,
                uint32_t val_cap, uint32_t start_op) {
  const size_t O = (size_t)n_ops + 1, R = (size_t)rows + 1;
  uint8_t* p = (uint8_t*)block;
  auto take = [&](size_t bytes) { void* r = p; p += al256(bytes); return r; };
  L.n_ops = n_ops; L.n_values = n_values; L.n_preds = n_preds; L.n_actors = n_actors; L.rows = rows; L.pred_rows = pred_rows; L.str_len = str_len; L.val_cap = val_cap;
  L.start_op = start_op;
  L.ops = (am355_local_op*)take(sizeof(am355_local_op) * O);
  L.values = (am355_local_value*)take(sizeof(am355_local_value) * ((size_t)n_values + 1));
  L.preds = (am355_local_pred*)take(sizeof(am355_local_pred) * ((size_t)n_preds + 1));
  L.rank = (uint32_t*)take(4 * ((size_t)n_actors + 1));
  L.multi = (uint32_t*)take(4 * O); L.pcnt = (uint32_t*)take(4 * O);
  L.arena = (uint8_t*)p;
  L.up_bytes = (size_t)(p - (uint8_t*)block) + str_len;
  (void)take((size_t)str_len + val_cap + 16);
  L.row_base = (uint32_t*)take(4 * O); L.pred_base = (uint32_t*)take(4 * O);
  L.vidx = (uint32_t*)take(4 * R); L.vlen = (uint32_t*)take(4 * R); L.voff = (uint32_t*)take(4 * R);
  L.scan_ws = take(2 * scan_workspace_bytes((uint32_t)std::max(O, R)));
}

__device__ __forceinline__ uint32_t local_uleb_len(unsigned long long v) { uint32_t n = 1; while (v >= 0x80) { v >>= 7; n++; } return n; }
__device__ __forceinline__ uint32_t local_sleb_len(long long v) {
  for (uint32_t n = 1;; n++) {
    const uint32_t b = (uint32_t)(v & 0x7f);
    v >>= 7;
    if ((v == 0 && !(b & 0x40)) || (v == -1 && (b & 0x40))) return n;
  }
}
// bytes a value takes in valRaw (columnar.js:259-292: Uint53 / Int53 as LEB128, a float64 as its 8 bytes, a string as its UTF-8)
__device__ __forceinline__ uint32_t local_value_len(const am355_local_value& v) {
  switch (v.tag) {
    case AM355_LV_UINT: return local_uleb_len(v.payload);
    case AM355_LV_INT: case AM355_LV_COUNTER: case AM355_LV_TIMESTAMP: return local_sleb_len((long long)v.payload);
    case AM355_LV_FLOAT64: return 8;
    case AM355_LV_UTF8: return v.len;
    default: return 0;
  }
}

// One ROW of the expanded change (columnar.js:446-475): the request op that owns the row by binary search over the scan of `multi`
// (row_base), then the row's fields as encodeOps appends them (:397-428). Shared by kl_expand and kl_small.
struct LocalRow {
  uint32_t obj_actor, obj_ctr, key_actor, key_ctr, key_off, key_len, insert, action;
  uint32_t vidx, vlen, val_tl;     // value record of the row (NONE32: none) | its bytes in valRaw | length << 4 | tag
  uint32_t pred_at, pred_num;      // the row's entries in the pred columns
  uint32_t k;                      // the row's place inside its op
  bool multi_del;
};
__device__ __forceinline__ LocalRow local_expand_row(const LocalBufs& L, const uint32_t* row_base, const uint32_t* pred_base, uint32_t row, am355_local_op& op) {
  uint32_t lo = 0, hi = L.n_ops;   // the last op whose first row is <= row (ops without rows share their successor's first row)
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (row_base[mid] <= row) lo = mid; else hi = mid;
  }
  op = L.ops[lo];
  LocalRow r;
  r.k = row - row_base[lo];
  const bool multi_ins = op.action == 1 && (op.flags & AM355_LOP_VALUES) && (op.flags & AM355_LOP_INSERT);
  r.multi_del = op.action == 3 && op.multi > 1;
  r.key_actor = NONE32; r.key_ctr = NONE32; r.key_off = 0; r.key_len = NONE32;
  if (op.key_kind == AM355_LK_STRING) { r.key_off = op.key_off; r.key_len = op.key_len; }
  else if (op.key_kind == AM355_LK_HEAD) r.key_ctr = 0;
  else { r.key_actor = op.elem_actor; r.key_ctr = op.elem_ctr; }
  if (multi_ins && r.k > 0) { r.key_actor = 0; r.key_ctr = L.start_op + row - 1; }   // behind the value in front of it: the id of the row before (:457)
  if (r.multi_del) r.key_ctr += r.k;                                                  // (:464)
  r.obj_actor = op.obj_actor;
  r.obj_ctr = op.obj_actor == NONE32 ? NONE32 : op.obj_ctr;
  r.insert = (op.flags & AM355_LOP_INSERT) ? 1 : 0;
  r.action = op.action;
  r.vidx = NONE32; r.vlen = 0; r.val_tl = 0;
  if (op.action == 1 || op.action == 5) {
    r.vidx = op.val_first + (multi_ins ? r.k : 0);
    const am355_local_value v = L.values[r.vidx];
    r.vlen = local_value_len(v);
    r.val_tl = r.vlen << 4 | v.tag;
  }
  r.pred_at = pred_base[lo] + (r.multi_del ? r.k : 0);
  r.pred_num = multi_ins ? 0u : r.multi_del ? 1u : op.pred_num;
  return r;
}

// The row's pred entries into p_actor / p_ctr[0 .. r.pred_num), in (counter, actor id) order: compareParsedOpIds compares the id
// STRINGS, so by the table's ranks, not by local number (:394-396, :423; a multiOp deletion: its one pred counted up, :465)
__device__ __forceinline__ void local_row_preds(const LocalBufs& L, const am355_local_op& op, const LocalRow& r, uint32_t* p_actor, uint32_t* p_ctr) {
  if (r.multi_del) { p_actor[0] = L.preds[op.pred_first].actor; p_ctr[0] = L.preds[op.pred_first].ctr + r.k; return; }
  for (uint32_t i = 0; i < r.pred_num; i++) {
    const am355_local_pred pr = L.preds[op.pred_first + i];
    const unsigned long long key = (unsigned long long)pr.ctr << 32 | L.rank[pr.actor];
    uint32_t j = i;
    for (; j > 0; j--) {
      const uint32_t qa = p_actor[j - 1], qc = p_ctr[j - 1];
      if (((unsigned long long)qc << 32 | L.rank[qa]) <= key) break;
      p_actor[j] = qa; p_ctr[j] = qc;
    }
    p_actor[j] = pr.actor; p_ctr[j] = pr.ctr;
  }
}

// the `len` bytes of a value as valRaw holds them (columnar.js:259-292)
__device__ __forceinline__ void local_value_write(const LocalBufs& L, const am355_local_value& v, uint32_t len, uint8_t* out) {
  if (v.tag == AM355_LV_UTF8) {
    const uint8_t* src = L.arena + v.off;
    for (uint32_t i = 0; i < len; i++) out[i] = src[i];
  } else if (v.tag == AM355_LV_FLOAT64) {
    for (uint32_t i = 0; i < 8; i++) out[i] = (uint8_t)(v.payload >> (8 * i));
  } else if (v.tag == AM355_LV_UINT) {
    unsigned long long x = v.payload;
    for (uint32_t i = 0; i < len; i++) { out[i] = (uint8_t)((x & 0x7f) | (i + 1 < len ? 0x80 : 0)); x >>= 7; }
  } else {
    long long x = (long long)v.payload;
    for (uint32_t i = 0; i < len; i++) { out[i] = (uint8_t)((x & 0x7f) | (i + 1 < len ? 0x80 : 0)); x >>= 7; }
  }
}

// One thread per ROW of the expanded change. Row `rows` (one past the end) closes the value-length array.
__global__ __launch_bounds__(BLOCK) void kl_expand(LocalBufs L, HistBufs h) {
  const uint32_t row = gtid();
  if (row > L.rows) return;
  if (row == L.rows) { L.vlen[row] = 0; L.vidx[row] = NONE32; return; }
  am355_local_op op;
  const LocalRow r = local_expand_row(L, L.row_base, L.pred_base, row, op);
  h.v_obj_actor[row] = r.obj_actor; h.v_obj_ctr[row] = r.obj_ctr;
  h.v_key_actor[row] = r.key_actor; h.v_key_ctr[row] = r.key_ctr; h.v_key_off[row] = r.key_off; h.v_key_len[row] = r.key_len;
  h.v_insert[row] = (uint8_t)r.insert;
  h.v_action[row] = r.action;
  h.v_val_tl[row] = r.val_tl;
  h.v_val_off[row] = 0;   // (kl_values, once the lengths are scanned)
  L.vidx[row] = r.vidx; L.vlen[row] = r.vlen;
  h.v_pred_num[row] = r.pred_num;
  local_row_preds(L, op, r, h.p_actor + r.pred_at, h.p_ctr + r.pred_at);
}

// One thread per row: the value's bytes into the value arena at the scanned offset
__global__ __launch_bounds__(BLOCK) void kl_values(LocalBufs L, HistBufs h) {
  const uint32_t row = gtid();
  if (row >= L.rows) return;
  const uint32_t len = L.vlen[row], vi = L.vidx[row];
  if (!len || vi == NONE32) return;
  const uint32_t at = L.voff[row];
  if ((unsigned long long)at + len > L.val_cap) { atomicOr(&h.flags[0], (uint32_t)HF_INVALID); return; }   // (the host sized the arena from the same values)
  h.v_val_off[row] = L.str_len + at;
  local_value_write(L, L.values[vi], len, L.arena + L.str_len + at);
}

void local_expand_encode(const LocalBufs& L, HistBufs& h, hipStream_t st) {
  const uint32_t M = L.rows;
  (void)hipMemsetAsync(h.flags, 0, 16, st);
  (void)hipMemsetAsync(h.col_len, 0, 4 * HIST_NCOL, st);
  if (!M) return;
  (void)hipMemsetAsync(h.seg, 0, 4 * (size_t)M, st);   // one change: every row and every pred entry in segment 0
  if (L.pred_rows) (void)hipMemsetAsync(h.pseg, 0, 4 * (size_t)L.pred_rows, st);
  exclusive_scan2_u32(L.multi, L.row_base, nullptr, L.pcnt, L.pred_base, nullptr, L.n_ops + 1, L.scan_ws, st);
  AM355_LAUNCH_INDEPENDENT(kl_expand, grid_for(M + 1), dim3(BLOCK), st, L, h);
  exclusive_scan_u32(L.vlen, L.voff, M + 1, nullptr, L.scan_ws, st);
  AM355_LAUNCH_INDEPENDENT(kl_values, grid_for(M), dim3(BLOCK), st, L, h);
  h.P = L.pred_rows;
  hist_encode_columns(L.arena, h, M, st, [](int, bool, bool, uint32_t) {});
}

// ---------------------------------------------------------------------------------------------------------
// a SMALL local change in one workgroup (am355_set_local_small; am355_hist.h LOCAL_SMALL_*)
// ---------------------------------------------------------------------------------------------------------
// The bulk path above is ~115 stream commands for a typed character: launch gaps over a handful of values. Here ONE workgroup of twelve
// wavefronts does the whole build: the two scans, the expansion (one row per thread, local_expand_row), then ONE WAVEFRONT PER COLUMN.
// The twelve columns are independent of each other, so no column waits for another; a wavefront walks its column 64 values at a time.
// What the reference's encoder state machine emits is a function of the value sequence alone (am355_encode.hip), and every piece of it
// follows from three bit masks of the column, which a ballot per 64 values gives: which values are non-null, which start a run, and
// from the two which are LONE (a run of one non-null value):
//   a run starts where the value differs from the one before; its length = distance to the next start bit;
//   a null run is (0, n); a run of >= 2 equal values (n, v); a maximal stretch of lone values ONE literal (-k, v1..vk), whose count k =
//   distance to the next clear bit of the lone mask -- no look-ahead state is carried, the masks of the whole column sit in LDS;
//   delta columns: the value in front of a non-null value = the next lower bit of the non-null mask.
// Sizes are scanned per wavefront (six __shfl_up steps per 64 values, the carry by lane broadcast), the twelve lengths by one thread, and
// every run writes its bytes into the column's stretch of ONE LDS byte arena, columns back to back. The arena, the twelve lengths and
// the flag word then go to pinned host memory as plain dword stores. Each size / write rule is stated once: ls_run<false> counts,
// ls_run<true> writes.
constexpr uint32_t LS_THREADS = HIST_NCOL * WAVE;   // 768: a wavefront per column; >= LOCAL_SMALL_ROWS and > LOCAL_SMALL_OPS: a thread per row / per op
constexpr uint32_t LS_MAXN = LOCAL_SMALL_ROWS > LOCAL_SMALL_PREDS ? LOCAL_SMALL_ROWS : LOCAL_SMALL_PREDS;
constexpr uint32_t LS_WORDS = LS_MAXN / 64 + 1;     // 64-bit words of a column's masks: a bit per value and the closing bit at n
static_assert(LOCAL_SMALL_ROWS <= LS_THREADS && LOCAL_SMALL_OPS + 1 <= LS_THREADS, "a thread per row and per op");
static_assert(LOCAL_SMALL_OUT_BYTES % 4 == 0 && LOCAL_SMALL_HEAD >= 4 * (4 + HIST_NCOL), "pinned layout of kl_small");
enum : uint32_t { LS_V_KEY_OFF = 4, LS_V_KEY_LEN = 5, LS_V_VIDX = 8 };   // s.v[k]: column k's values, except: 4 / 5 the key's range, 8 the value record
enum : uint32_t { LS_NUM = 0, LS_DELTA = 1, LS_STR = 2, LS_BOOL = 3, LS_RAW = 4 };

struct LsLds {
  alignas(16) uint8_t out[LOCAL_SMALL_OUT_BYTES];     // the twelve columns back to back
  uint32_t v[10][LOCAL_SMALL_ROWS];                    // by row
  uint32_t p[2][LOCAL_SMALL_PREDS];                    // by pred entry: actor | counter
  uint32_t d[2][LS_MAXN];                              // deltas of keyCtr | of predCtr
  uint32_t off[HIST_NCOL][LS_MAXN];                    // byte offset of the run that starts at value i, inside its column
  unsigned long long nn[HIST_NCOL][LS_WORDS], start[HIST_NCOL][LS_WORDS];
  uint32_t row_base[LOCAL_SMALL_OPS + 1], pred_base[LOCAL_SMALL_OPS + 1];
  uint32_t wtot[LS_THREADS / WAVE], col_len[HIST_NCOL], col_base[HIST_NCOL + 1], flag;
  uint8_t ins[LOCAL_SMALL_ROWS];
};
static_assert(sizeof(LsLds) <= 132 * 1024, "LDS of kl_small: the 160 KB of a gfx950 workgroup with room to spare");

// exclusive prefix of v over the LS_THREADS threads; *total = their sum. Every thread must call it.
__device__ __forceinline__ uint32_t ls_block_scan(uint32_t v, uint32_t* wtot, uint32_t* total) {
  const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const uint32_t incl = wave_incl_scan_u32(v, lane);
  if (lane == WAVE - 1) wtot[w] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t k = 0; k < LS_THREADS / WAVE; k++) {
    const uint32_t x = wtot[k];
    before += k < w ? x : 0;
    all += x;
  }
  __syncthreads();
  *total = all;
  return before + incl - v;
}

// ---- the masks of one column: nw words are written; bit n (the closing start bit) lies inside them ----
__device__ __forceinline__ bool ls_bit(const unsigned long long* m, uint32_t i) { return (m[i >> 6] >> (i & 63)) & 1; }
// first set bit at or behind `from` (the closing bit ends the search)
__device__ __forceinline__ uint32_t ls_next_set(const unsigned long long* m, uint32_t nw, uint32_t from) {
  uint32_t k = from >> 6;
  unsigned long long w = m[k] & (~0ull << (from & 63));
  while (!w) {
    if (++k >= nw) return nw * 64;
    w = m[k];
  }
  return k * 64 + (uint32_t)__ffsll(w) - 1;
}
// last set bit in front of i (NONE32: none)
__device__ __forceinline__ uint32_t ls_prev_set(const unsigned long long* m, uint32_t i) {
  uint32_t k = i >> 6;
  unsigned long long w = (i & 63) ? m[k] & ((1ull << (i & 63)) - 1) : 0ull;
  while (!w) {
    if (k == 0) return NONE32;
    w = m[--k];
  }
  return k * 64 + 63 - (uint32_t)__clzll(w);
}
// lone values: a run starts here, the next starts right behind, and the value is not null
__device__ __forceinline__ unsigned long long ls_lone_word(const unsigned long long* start, const unsigned long long* nn, uint32_t nw, uint32_t k) {
  const unsigned long long behind = (start[k] >> 1) | ((k + 1 < nw ? start[k + 1] : 0ull) << 63);
  return start[k] & nn[k] & behind;
}
__device__ __forceinline__ bool ls_lone(const unsigned long long* start, const unsigned long long* nn, uint32_t nw, uint32_t i) {
  return (ls_lone_word(start, nn, nw, i >> 6) >> (i & 63)) & 1;
}
// first value at or behind i that is not lone (the closing position n is not)
__device__ __forceinline__ uint32_t ls_next_not_lone(const unsigned long long* start, const unsigned long long* nn, uint32_t nw, uint32_t i) {
  uint32_t k = i >> 6;
  unsigned long long w = ~ls_lone_word(start, nn, nw, k) & (~0ull << (i & 63));
  while (!w) {
    if (++k >= nw) return nw * 64;
    w = ~ls_lone_word(start, nn, nw, k);
  }
  return k * 64 + (uint32_t)__ffsll(w) - 1;
}

// counting (W = false) or writing (W = true) emitters: both return the bytes
template <bool W> __device__ __forceinline__ uint32_t ls_uleb(uint8_t*& p, uint64_t v) {
  const uint32_t n = uleb_size(v);
  if (W) p = put_uleb(p, v);
  return n;
}
template <bool W> __device__ __forceinline__ uint32_t ls_sleb(uint8_t*& p, int64_t v) {
  const uint32_t n = sleb_size(v);
  if (W) p = put_sleb(p, v);
  return n;
}

// one column as its wavefront sees it. nul: NONE32 there = the value is null (nullptr: never null); val: what is compared and written
struct LsCol {
  uint32_t kind, n;
  const uint32_t *nul, *val;
  const uint8_t* ins;
};
__device__ __forceinline__ bool ls_is_null(const LsCol& q, uint32_t i) { return q.nul && q.nul[i] == NONE32; }
// does value i (> 0) continue the run of value i - 1?
__device__ __forceinline__ bool ls_same(const LsCol& q, const LocalBufs& L, const uint32_t* key_off, uint32_t i) {
  if (q.kind == LS_RAW) return false;
  if (q.kind == LS_BOOL) return (q.ins[i] != 0) == (q.ins[i - 1] != 0);
  const bool ni = ls_is_null(q, i), nj = ls_is_null(q, i - 1);
  if (ni != nj) return false;
  if (ni) return true;
  if (q.kind != LS_STR) return q.val[i] == q.val[i - 1];
  const uint32_t len = q.nul[i];
  if (len != q.nul[i - 1]) return false;
  if (key_off[i] == key_off[i - 1]) return true;
  const uint8_t *a = L.arena + key_off[i], *b = L.arena + key_off[i - 1];
  for (uint32_t k = 0; k < len; k++)
    if (a[k] != b[k]) return false;
  return true;
}
// the value of a run, as the column writes it
template <bool W> __device__ __forceinline__ uint32_t ls_value(const LsCol& q, const LocalBufs& L, const uint32_t* key_off, uint32_t i, uint8_t*& p) {
  if (q.kind == LS_DELTA) return ls_sleb<W>(p, (int64_t)(int32_t)q.val[i]);
  if (q.kind == LS_NUM) return ls_uleb<W>(p, q.val[i]);
  const uint32_t len = q.nul[i];   // (LS_STR: the length prefix and the key's bytes)
  const uint32_t n = ls_uleb<W>(p, len) + len;
  if (W) {
    const uint8_t* a = L.arena + key_off[i];
    for (uint32_t k = 0; k < len; k++) p[k] = a[k];
    p += len;
  }
  return n;
}
// The run that starts at value i: its bytes, counted or written at p. `any`: the column holds a value that is not null (a column of
// nothing but nulls is empty, encoding.js:651-654).
template <bool W>
__device__ __forceinline__ uint32_t ls_run(const LsCol& q, const LocalBufs& L, const LsLds& s, uint32_t c, uint32_t nw, bool any, uint32_t i, uint8_t* p) {
  const unsigned long long *start = s.start[c], *nn = s.nn[c];
  if (q.kind == LS_RAW) {   // the value bytes of row i (raw values: no headers)
    const uint32_t len = s.v[7][i] >> 4;
    if (W && len) local_value_write(L, L.values[s.v[LS_V_VIDX][i]], len, p);
    return len;
  }
  const uint32_t len = ls_next_set(start, nw, i + 1) - i;
  if (q.kind == LS_BOOL) {   // alternating run lengths, the first run counts `false` (encoding.js:1061-1135)
    uint32_t sz = 0;
    if (i == 0 && q.ins[0]) { if (W) *p++ = 0; sz = 1; }
    return sz + ls_uleb<W>(p, len);
  }
  if (!any) return 0;
  if (ls_is_null(q, i)) {
    if (W) *p++ = 0;
    return 1 + ls_uleb<W>(p, len);
  }
  uint32_t sz = 0;
  if (len >= 2) sz = ls_sleb<W>(p, (int64_t)len);
  else if (i == 0 || !ls_lone(start, nn, nw, i - 1)) sz = ls_sleb<W>(p, -(int64_t)(ls_next_not_lone(start, nn, nw, i) - i));   // the literal's count
  return sz + ls_value<W>(q, L, s.v[LS_V_KEY_OFF], i, p);
}

__global__ __launch_bounds__(LS_THREADS) void kl_small(LocalBufs L, uint8_t* host_out) {
  __shared__ LsLds s;
  const uint32_t t = threadIdx.x, lane = t & (WAVE - 1), c = t / WAVE;
  const uint32_t M = L.rows, P = L.pred_rows, O = L.n_ops;
  uint32_t* h_words = (uint32_t*)host_out;   // flags[4] | col_len[HIST_NCOL]
  auto refuse = [&]() {   // (every thread takes the same way out)
    if (t < 4) h_words[t] = t == 0 ? (uint32_t)HF_INVALID : 0u;
    if (t < HIST_NCOL) h_words[4 + t] = 0;
  };
  if (M > LOCAL_SMALL_ROWS || P > LOCAL_SMALL_PREDS || O > LOCAL_SMALL_OPS) { refuse(); return; }   // (the host asked local_small_fits first)
  if (t == 0) s.flag = 0;
  // ---- the scans over `multi` and `pcnt`: first row / first pred entry of every op ----
  uint32_t rows = 0, preds = 0;
  const uint32_t rb = ls_block_scan(t < O ? L.multi[t] : 0u, s.wtot, &rows);
  const uint32_t pb = ls_block_scan(t < O ? L.pcnt[t] : 0u, s.wtot, &preds);
  if (t <= O) { s.row_base[t] = rb; s.pred_base[t] = pb; }
  if (rows != M || preds != P) { refuse(); return; }   // the counts the host planned with are not what the ops expand to
  __syncthreads();
  // ---- expansion: a thread per row ----
  if (t < M) {
    am355_local_op op;
    const LocalRow r = local_expand_row(L, s.row_base, s.pred_base, t, op);
    s.v[0][t] = r.obj_actor; s.v[1][t] = r.obj_ctr; s.v[2][t] = r.key_actor; s.v[3][t] = r.key_ctr;
    s.v[LS_V_KEY_OFF][t] = r.key_off; s.v[LS_V_KEY_LEN][t] = r.key_len;
    s.v[6][t] = r.action; s.v[7][t] = r.val_tl; s.v[LS_V_VIDX][t] = r.vidx; s.v[9][t] = r.pred_num;
    s.ins[t] = (uint8_t)r.insert;
    if ((unsigned long long)r.pred_at + r.pred_num > P) atomicOr(&s.flag, (uint32_t)HF_INVALID);
    else local_row_preds(L, op, r, s.p[0] + r.pred_at, s.p[1] + r.pred_at);
  }
  __syncthreads();
  if (s.flag) { refuse(); return; }
  // ---- a wavefront per column ----
  LsCol q;
  q.kind = c == 3 || c == 11 ? LS_DELTA : c == 4 ? LS_STR : c == 5 ? LS_BOOL : c == 8 ? LS_RAW : LS_NUM;
  q.n = c >= 10 ? P : M;
  q.nul = c == 4 ? s.v[LS_V_KEY_LEN] : c == 5 || c == 8 ? nullptr : c == 10 ? s.p[0] : c == 11 ? s.p[1] : s.v[c];
  q.val = c == 3 ? s.d[0] : c == 11 ? s.d[1] : q.nul;
  q.ins = s.ins;
  const uint32_t n = q.n, nw = (M > P ? M : P) / 64 + 1;   // the same trip count for every wavefront: the barriers below are the workgroup's
  bool any = false;
  for (uint32_t ch = 0; ch < nw; ch++) {
    const uint32_t i = ch * 64 + lane;
    const unsigned long long m = __ballot(i < n && !ls_is_null(q, i));
    if (lane == 0) s.nn[c][ch] = m;
    any = any || m != 0;
  }
  __syncthreads();
  if (q.kind == LS_DELTA) {   // successive differences of the values that are not null (encoding.js:932-948), modulo 2^32: exact int32
    uint32_t* d = c == 3 ? s.d[0] : s.d[1];
    for (uint32_t i = lane; i < n; i += WAVE) {
      if (q.nul[i] == NONE32) { d[i] = 0; continue; }
      const uint32_t j = ls_prev_set(s.nn[c], i);
      d[i] = q.nul[i] - (j != NONE32 ? q.nul[j] : 0u);
    }
  }
  __syncthreads();
  for (uint32_t ch = 0; ch < nw; ch++) {
    const uint32_t i = ch * 64 + lane;
    const unsigned long long m = __ballot(i < n ? (i == 0 || !ls_same(q, L, s.v[LS_V_KEY_OFF], i)) : i == n);
    if (lane == 0) s.start[c][ch] = m;
  }
  __syncthreads();
  uint32_t carry = 0;
  for (uint32_t ch = 0; ch < nw; ch++) {
    const uint32_t i = ch * 64 + lane;
    const uint32_t sz = i < n && ls_bit(s.start[c], i) ? ls_run<false>(q, L, s, c, nw, any, i, nullptr) : 0u;
    const uint32_t incl = wave_incl_scan_u32(sz, lane);
    if (i < n) s.off[c][i] = carry + incl - sz;
    carry += __shfl(incl, WAVE - 1);
  }
  if (lane == 0) s.col_len[c] = carry;
  __syncthreads();
  if (t == 0) {
    uint32_t at = 0;
    for (uint32_t k = 0; k < HIST_NCOL; k++) { s.col_base[k] = at; at += s.col_len[k]; }
    s.col_base[HIST_NCOL] = at;
    if (at > LOCAL_SMALL_OUT_BYTES) s.flag = HF_INVALID;   // (cannot be for a request inside the limits: the arena is their worst case)
  }
  __syncthreads();
  if (s.flag) { refuse(); return; }
  for (uint32_t i = lane; i < n; i += WAVE) {
    if (!ls_bit(s.start[c], i)) continue;
    // the run's stretch: up to where the next run starts, inside the column's stretch, inside the arena
    const uint32_t j = ls_next_set(s.start[c], nw, i + 1), end = j < n ? s.off[c][j] : s.col_len[c];
    if (s.off[c][i] > end || (size_t)s.col_base[c] + end > LOCAL_SMALL_OUT_BYTES) { atomicOr(&s.flag, (uint32_t)HF_INVALID); continue; }
    if (end > s.off[c][i]) (void)ls_run<true>(q, L, s, c, nw, any, i, s.out + s.col_base[c] + s.off[c][i]);
  }
  __syncthreads();
  if (s.flag) { refuse(); return; }
  // ---- to the host: the bytes as dwords, the lengths, the flag word ----
  const uint32_t words = (s.col_base[HIST_NCOL] + 3) / 4;
  uint32_t* dst = (uint32_t*)(host_out + LOCAL_SMALL_HEAD);
  const uint32_t* src = (const uint32_t*)s.out;
  for (uint32_t w = t; w < words; w += LS_THREADS) dst[w] = src[w];
  if (t < HIST_NCOL) h_words[4 + t] = s.col_len[t];
  if (t < 4) h_words[t] = 0;
}

void local_small_encode(const LocalBufs& L, uint8_t* host_out, hipStream_t st) {
  hipLaunchKernelGGL(kl_small, dim3(1), dim3(LS_THREADS), 0, st, L, host_out);
}

}  // namespace am355
