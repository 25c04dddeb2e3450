// The string of a Text object read straight from the whole-document edit records in HBM (include/am355.h: am355_object_text): what the
// reference's frontend shows as Text.toString() after applyPatch(getPatch(state)), without the patch. PatchIR.edit holds one record per
// typed run and a record's bytes lie back to back in the arena, so the text is a filtered, scanned gather of arena stretches: it moves
// as many bytes as the string has.
//
// THE RULE (frontend/apply_patch.js:231-255 updateTextObject, frontend/text.js:64-67 toString):
//   1. One element per list index: `insert` / `multi-insert` edits splice elements in (apply_patch.js:232-245).
//   2. Where an element shows several values (its insert plus updates, or updates only behind a row without a value), every `update`
//      replaces the element at its index (apply_patch.js:247-250): the last `update` of that index wins.
//   3. toString concatenates the elements whose value is a JS string (text.js:64-67): values of type UTF8, val_tl & 15 == 6
//      (columnar.js:47-48).
//   4. Numbers, booleans, null, bytes, child objects (AM355_EDIT_CHILD), counter totals (AM355_EDIT_COUNTER) and `remove` records
//      (AM355_EDIT_REMOVE; apply_patch.js:252-253 splices nothing out of a list that is being built) contribute nothing.
//   5. Every such element except a `remove` record still counts in the length (n_elements).
//
// ON THE RECORD TABLE (am355_textrec.h, which proves it): only the last value of a record can be overwritten, only by the record directly
// behind it, and it is iff that record belongs to the same object, carries AM355_EDIT_UPDATE and has index == record.index + count - 1.
//
// A LEADING U+FEFF: the reference decodes every value by itself with TextDecoder('utf-8') (encoding.js:9-17), which drops a leading byte
// order mark; a value whose bytes begin EF BB BF contributes without them (am355_render.cpp prim_value does the same). Such values
// break "a record is one stretch of the arena": kt_sizes marks their record (TM_BOM) and kt_gather walks a marked record value by value,
// from its first value on for every 16 bytes of output -- which is why a marked record of more than TEXT_BOM_WALK_MAX values is left
// to the caller's own path (AM355_E_UNSUPPORTED): a text with byte order marks INSIDE a typed run of thousands of characters is not
// something an editor produces, and a bounded walk keeps the worst case of the kernel bounded.
//
// Included at the end of am355_calls.hip, not compiled by itself.
#include "am355_textrec.h"

namespace am355 {

constexpr uint32_t TEXT_CHUNK = 16;                                    // output bytes a thread owns: one 16-byte store
constexpr uint32_t TEXT_WG_BYTES = BLOCK * TEXT_CHUNK;                 // output bytes one kt_gather workgroup owns (4 KiB: 1 MB of text fills the 256 CUs once)
constexpr uint32_t TEXT_BOM_INLINE = 32;                               // values of a record its own kt_sizes thread looks at; more: the workgroup does
constexpr uint32_t TEXT_BOM_WALK_MAX = 4096;                           // values of a record with byte order marks kt_gather walks
enum TextMark : uint8_t { TM_STRING = 1, TM_BOM = 2 };
constexpr uint32_t TF_BOM_LONG = RF_CALL;   // flag bit of a read: a record with byte order marks holds more than TEXT_BOM_WALK_MAX values

__device__ __forceinline__ bool text_bom_at(const uint8_t* __restrict__ p) { return p[0] == 0xef && p[1] == 0xbb && p[2] == 0xbf; }

// values of record k and how many of them stand: all, less the last one if the record behind overwrites it; 0 of a `remove` record.
// false: the record's `first` words are out of order or past the table.
__device__ __forceinline__ bool text_live(const TextRecs& t, uint32_t k, uint32_t& count, uint32_t& live) {
  live = 0;
  if (!rec_count(t, k, count)) return false;
  live = (t[k].flags & AM355_EDIT_REMOVE) ? 0u : count - (rec_overwritten(t, k, count) ? 1u : 0u);
  return true;
}

// Pass 1, one thread per record: bytes[k] = bytes the record contributes, elems[k] = elements it leaves in the list, mark[k] = TM_STRING
// | TM_BOM; the elements that are no strings are summed into words[TW_NONSTR]. A record of values of >= 3 bytes is looked at value by
// value for the byte order mark: up to TEXT_BOM_INLINE values by its own thread, a longer one (a pasted run of three-byte characters) by
// the whole workgroup, 256 values per step.
__global__ __launch_bounds__(BLOCK) void kt_sizes(TextRecs t, const uint8_t* __restrict__ arena, uint64_t arena_len, uint32_t* __restrict__ bytes,
                                                  uint32_t* __restrict__ elems, uint8_t* __restrict__ mark, uint32_t* __restrict__ words) {
  __shared__ uint32_t s_red[BLOCK / WAVE];
  __shared__ uint32_t s_n_long;
  __shared__ uint32_t s_owner[BLOCK], s_off[BLOCK], s_len[BLOCK], s_live[BLOCK];
  if (threadIdx.x == 0) s_n_long = 0;
  __syncthreads();
  const uint32_t k = gtid();
  uint32_t count = 0, live = 0, nbytes = 0, nonstr = 0, err = 0, boms = 0, len = 0;
  uint8_t m = 0;
  if (k < t.R) {
    const am355_ir_edit& rec = t[k];
    if (!text_live(t, k, count, live)) err |= RF_TABLE;
    const bool is_str = !(rec.flags & (AM355_EDIT_CHILD | AM355_EDIT_COUNTER | AM355_EDIT_REMOVE)) && (rec.val_tl & 15u) == 6u;
    if (!is_str) {
      nonstr = live;
    } else {
      len = rec.val_tl >> 4;
      if ((uint64_t)rec.val_off + (uint64_t)count * len > arena_len) {
        err |= RF_TABLE;   // (arena bytes outside the table; nothing of the record is read: bytes stay 0)
      } else {
        m = TM_STRING;
        nbytes = live * len;   // (distinct bytes of an arena of less than 4 GiB: the sum over the object fits 32 bits)
        if (len >= 3 && live) {
          if (live <= TEXT_BOM_INLINE) {
            for (uint32_t v = 0; v < live; v++) boms += text_bom_at(arena + rec.val_off + (size_t)v * len) ? 1u : 0u;
          } else {
            const uint32_t slot = atomicAdd(&s_n_long, 1u);
            s_owner[slot] = threadIdx.x; s_off[slot] = rec.val_off; s_len[slot] = len; s_live[slot] = live;
          }
        }
      }
    }
  }
  __syncthreads();
  const uint32_t n_long = s_n_long;
  for (uint32_t j = 0; j < n_long; j++) {   // (uniform over the workgroup: every thread reaches the sums)
    uint32_t part = 0;
    const uint32_t off = s_off[j], l = s_len[j], n = s_live[j];
    for (uint32_t v = threadIdx.x; v < n; v += BLOCK) part += text_bom_at(arena + off + (size_t)v * l) ? 1u : 0u;
    const uint32_t all = block_sum_u32(part, s_red);
    if (s_owner[j] == threadIdx.x) boms = all;
  }
  if (boms) {
    m |= TM_BOM;
    nbytes -= 3 * boms;
    if (live > TEXT_BOM_WALK_MAX) err |= TF_BOM_LONG;
  }
  if (k < t.R) { bytes[k] = nbytes; elems[k] = live; mark[k] = m; }
  const uint32_t wg_nonstr = block_sum_u32(nonstr, s_red);
  if (threadIdx.x == 0 && wg_nonstr) atomicAdd(&words[TW_NONSTR], wg_nonstr);
  if (err) atomicOr(&words[TW_FLAGS], err);
}

// Pass 3, parallel over the OUTPUT: a workgroup owns TEXT_WG_BYTES bytes, a thread TEXT_CHUNK of them (neighbouring threads write
// neighbouring 16-byte words; the binary search is a chain of dependent loads, so the more threads search side by side the better). It finds the record of its first byte by binary search over the scanned offsets (the last record
// that begins at or before it: the records of no bytes in between are passed over), and copies: one unaligned 16-byte load where the 16
// bytes lie in one unmarked record -- the case of a typed or pasted run --, byte by byte where records end inside them (a document typed
// character by character: sixteen records) or the record drops byte order marks. Always one aligned 16-byte store: the buffer is padded.
__global__ __launch_bounds__(BLOCK) void kt_gather(TextRecs t, const uint32_t* __restrict__ off, const uint8_t* __restrict__ mark, uint32_t total,
                                                   const uint8_t* __restrict__ arena, uint8_t* __restrict__ out) {
  {
    const uint32_t R = t.R;
    const uint64_t p64 = (uint64_t)blockIdx.x * TEXT_WG_BYTES + (uint64_t)threadIdx.x * TEXT_CHUNK;
    if (p64 >= total) return;
    const uint32_t p = (uint32_t)p64;
    uint32_t lo = 0, hi = R;   // off[lo] <= p < off[hi] (off[R]: total)
    while (hi - lo > 1) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (off[mid] <= p) lo = mid; else hi = mid;
    }
    uint32_t k = lo;
    uint32_t rec_end = k + 1 < R ? off[k + 1] : total;
    const uint32_t n = total - p < TEXT_CHUNK ? total - p : TEXT_CHUNK;
    uint4 w;
    w.x = w.y = w.z = w.w = 0u;
    if (n == TEXT_CHUNK && p + TEXT_CHUNK <= rec_end && !(mark[k] & TM_BOM)) {
      const U4 x = *(const U4*)(arena + t[k].val_off + (p - off[k]));
      w.x = x.x; w.y = x.y; w.z = x.z; w.w = x.w;
    } else {
      uint32_t rec_off = off[k], src = t[k].val_off;
      bool marked = (mark[k] & TM_BOM) != 0;
      // the cursor inside a marked record: value cur_v begins at contributed byte cur_base, its bytes at cur_src, cur_n of them
      uint32_t cur_v = 0, cur_base = 0, cur_src = 0, cur_n = 0, cur_live = 0, cur_len = 0;
      bool cur_set = false;
      uint32_t b4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (uint32_t j = 0; j < TEXT_CHUNK; j++) {
        if (j < n) {
          const uint32_t q = p + j;
          while (q >= rec_end) {   // (q < total: a record that holds q comes)
            k++;
            rec_off = rec_end;
            rec_end = k + 1 < R ? off[k + 1] : total;
            src = t[k].val_off;
            marked = (mark[k] & TM_BOM) != 0;
            cur_set = false;
          }
          uint32_t byte;
          if (!marked) {
            byte = arena[src + (q - rec_off)];
          } else {
            if (!cur_set) {
              uint32_t count;
              (void)text_live(t, k, count, cur_live);
              cur_len = t[k].val_tl >> 4;
              cur_v = 0; cur_base = 0; cur_src = src;
              cur_n = cur_len - (text_bom_at(arena + src) ? 3u : 0u);
              cur_set = true;
            }
            const uint32_t r = q - rec_off;
            while (r >= cur_base + cur_n && cur_v + 1 < cur_live) {
              cur_base += cur_n;
              cur_v++;
              cur_src = src + cur_v * cur_len;
              cur_n = cur_len - (text_bom_at(arena + cur_src) ? 3u : 0u);
            }
            byte = r - cur_base < cur_n ? arena[cur_src + (cur_len - cur_n) + (r - cur_base)] : 0u;
          }
          b4[j >> 2] |= byte << (8 * (j & 3));
        }
      }
      w.x = b4[0]; w.y = b4[1]; w.z = b4[2]; w.w = b4[3];
    }
    *(uint4*)(out + p) = w;
  }
}

}  // namespace am355

namespace {

int object_text_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const uint8_t** utf8, size_t* len, am355_text_info* info) {
  if (!c) return AM355_E_ARG;
  if (!utf8 || !len || (!obj_actor && actor_len)) return fail(c, AM355_E_ARG, "am355_object_text: null argument");
  TextObject o;
  { int orc = text_open(c, "am355_object_text", obj_ctr, obj_actor, actor_len, 0, &c->n_text_launches, o); if (orc) return orc; }
  hipStream_t st = c->stream;
  const uint32_t R = o.recs.R;
  am355_text_info ti{0, 0, 0};
  size_t total = 0;
  if (R) {
    // ---- pass 1 + the scan: sizes, offsets, totals ----
    const size_t b_words = carve_size(TW_WORDS, 4), b_arr = carve_size(R, 4), b_mark = carve_size(R, 1), b_ws = carve_round(scan_workspace_bytes(R));
    if (!c->d_text.ensure(b_words + 2 * b_arr + b_mark + b_ws)) return fail(c, AM355_E_NOMEM, "device allocation failed (text)");
    uint8_t* dp = c->d_text.as<uint8_t>();
    uint32_t* dw = (uint32_t*)dp;
    uint32_t* d_off = (uint32_t*)(dp + b_words);
    uint32_t* d_elems = (uint32_t*)(dp + b_words + b_arr);
    uint8_t* d_mark = dp + b_words + 2 * b_arr;
    void* d_ws = dp + b_words + 2 * b_arr + b_mark;
    HIPCHK(c, hipMemsetAsync(dw + TW_BYTES, 0, 4 * 4, st));
    hipLaunchKernelGGL(kt_sizes, dim3((R + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, o.recs, (const uint8_t*)c->mb.arena, (uint64_t)c->raw.size(), d_off, d_elems, d_mark, dw);
    exclusive_scan2_u32(d_off, d_off, dw + TW_BYTES, d_elems, d_elems, dw + TW_ELEMS, R, d_ws, st);
    c->n_text_launches += 3;
    // the one wait of the read itself: the totals size the output
    HIPCHK(c, c->text_sig.fetch(dw + TW_BYTES, 4, TW_BYTES, st));
    const uint32_t* hw = c->text_sig.words();
    const uint32_t tf = hw[TW_FLAGS];
    { int prc = text_premise_error(c, TC_READ, tf, o.index); if (prc) return prc; }
    if (tf & TF_BOM_LONG)
      return fail(c, AM355_E_UNSUPPORTED, "a run of more than %u values with byte order marks inside: read through the patch", TEXT_BOM_WALK_MAX);
    total = hw[TW_BYTES];
    ti.n_elements = hw[TW_ELEMS];
    ti.n_strings = hw[TW_ELEMS] - hw[TW_NONSTR];
    ti.bytes = total;
    if (hw[TW_NONSTR] > hw[TW_ELEMS] || total > c->raw.size()) return fail(c, AM355_E_DEVICE, "internal: totals of the text read are inconsistent");
    if (total) {
      // ---- pass 3 (+ the copy down): into pinned memory directly for short strings, else into HBM and one copy ----
      const size_t padded = (total + TEXT_CHUNK - 1) / TEXT_CHUNK * TEXT_CHUNK;
      if (!c->h_text.ensure(padded + 16)) return fail(c, AM355_E_NOMEM, "host allocation failed (text)");
      const bool direct = total <= c->text_pinned_max;
      if (!direct && !c->d_text_out.ensure(padded + 16)) return fail(c, AM355_E_NOMEM, "device allocation failed (text)");
      uint8_t* dst = direct ? c->h_text.as<uint8_t>() : c->d_text_out.as<uint8_t>();
      const uint32_t wgs = (uint32_t)((total + TEXT_WG_BYTES - 1) / TEXT_WG_BYTES);
      AM355_LAUNCH_INDEPENDENT(kt_gather, dim3(wgs), dim3(BLOCK), st, o.recs, (const uint32_t*)d_off, (const uint8_t*)d_mark, (uint32_t)total, (const uint8_t*)c->mb.arena, dst);
      c->n_text_launches++;
      if (!direct) HIPCHK(c, hipMemcpyAsync(c->h_text.p, dst, total, hipMemcpyDeviceToHost, st));
      int prc = text_poll(c);
      if (prc) return prc;
    }
  }
  if (!c->h_text.p && !c->h_text.ensure(16)) return fail(c, AM355_E_NOMEM, "host allocation failed (text)");
  *utf8 = c->h_text.as<uint8_t>();
  *len = total;
  if (info) *info = ti;
  c->n_text_served++;
  return AM355_OK;
}

}  // namespace

extern "C" int am355_object_text(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const uint8_t** utf8, size_t* len, am355_text_info* info) {
  return guarded(c, [&]() { return object_text_impl(c, obj_ctr, obj_actor, actor_len, utf8, len, info); });
}
extern "C" int am355_object_text_calls(const am355_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_text_served;
  out[1] = c->n_text_launches;
  return AM355_OK;
}
extern "C" int am355_text_limits(uint32_t out[4]) {
  if (!out) return AM355_E_ARG;
  out[0] = TEXT_WG_BYTES; out[1] = BLOCK; out[2] = TEXT_BOM_INLINE; out[3] = TEXT_BOM_WALK_MAX;
  return AM355_OK;
}
extern "C" int am355_set_text_pinned_max(am355_ctx* c, uint64_t bytes) {
  if (!c) return AM355_E_ARG;
  c->text_pinned_max = (size_t)bytes;
  return AM355_OK;
}
