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
// ON THE RECORD TABLE: only the last value of a record can be overwritten, only by the record directly behind it, and it is iff that
// record belongs to the same object, carries AM355_EDIT_UPDATE and has index == record.index + count - 1. Why (am355_merge.hip
// list_edits_of, k_edit_runs, k_edit_pack):
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
//       type/length word or a gap in the arena), not its values; their index is the index of their first value (k_edit_pack).
//   (e) k_edit_pack gives every list object the records [edit_begin, edit_end) and nothing else, so "belongs to the same object" is
//       k + 1 < edit_end.
//
// A LEADING U+FEFF: the reference decodes every value by itself with TextDecoder('utf-8') (encoding.js:9-17), which drops a leading byte
// order mark; a value whose bytes begin EF BB BF contributes without them (am355_render.cpp prim_value does the same). Such values
// break "a record is one stretch of the arena": kt_sizes marks their record (TM_BOM) and kt_gather walks a marked record value by value,
// from its first value on for every 16 bytes of output -- which is why a marked record of more than TEXT_BOM_WALK_MAX values is left
// to the caller's own path (AM355_E_UNSUPPORTED): a text with byte order marks INSIDE a typed run of thousands of characters is not
// something an editor produces, and a bounded walk keeps the worst case of the kernel bounded.
//
// Included at the end of am355_calls.hip (behind am355_graph.hip), not compiled by itself.
#include "am355_ctx.h"

namespace am355 {

constexpr uint32_t TEXT_CHUNK = 16;                                    // output bytes a thread owns: one 16-byte store
constexpr uint32_t TEXT_WG_BYTES = BLOCK * TEXT_CHUNK;                 // output bytes one kt_gather workgroup owns (4 KiB: 1 MB of text fills the 256 CUs once)
constexpr uint32_t TEXT_BOM_INLINE = 32;                               // values of a record its own kt_sizes thread looks at; more: the workgroup does
constexpr uint32_t TEXT_BOM_WALK_MAX = 4096;                           // values of a record with byte order marks kt_gather walks
enum TextMark : uint8_t { TM_STRING = 1, TM_BOM = 2 };
// device words of a call (d_text): what kt_find found, then the totals and the flag word of kt_sizes
enum TextWord { TW_INDEX = 0, TW_TYPE = 1, TW_BEGIN = 2, TW_END = 3, TW_BYTES = 4, TW_ELEMS = 5, TW_NONSTR = 6, TW_FLAGS = 7, TW_WORDS = 8 };
enum TextFlag : uint32_t { TF_RANGE = 1,      // a record names values or arena bytes outside the tables
                           TF_BOM_LONG = 2 }; // a record with byte order marks holds more than TEXT_BOM_WALK_MAX values

// One thread per object: the object with that id leaves its index, type and edit range. (_root, index 0, has no id.)
__global__ __launch_bounds__(BLOCK) void kt_find(const am355_ir_object* __restrict__ obj, uint32_t n_obj, uint32_t ctr, uint32_t actor, uint32_t* __restrict__ words) {
  const uint32_t i = gtid();
  if (i == 0 || i >= n_obj) return;
  if (obj[i].id_ctr != ctr || obj[i].id_actor != actor) return;
  words[TW_INDEX] = i;
  words[TW_TYPE] = obj[i].type;
  words[TW_BEGIN] = obj[i].edit_begin;
  words[TW_END] = obj[i].edit_end;
}

__device__ __forceinline__ bool text_bom_at(const uint8_t* __restrict__ p) { return p[0] == 0xef && p[1] == 0xbb && p[2] == 0xbf; }

// values of record k (of the R records from `begin` on) and how many of them stand: all, less the last one if the record behind
// overwrites it (the rule above); 0 of a `remove` record. false: the record's `first` words are out of order or past the table.
__device__ __forceinline__ bool text_live(const am355_ir_edit* __restrict__ edit, uint32_t begin, uint32_t R, uint32_t k, uint32_t n_values, uint32_t& count, uint32_t& live) {
  const am355_ir_edit& rec = edit[begin + k];
  const am355_ir_edit& nxt = edit[begin + k + 1];   // (the table ends with a sentinel record: k + 1 <= n_erecs)
  count = live = 0;
  if (nxt.first <= rec.first || nxt.first > n_values) return false;
  count = nxt.first - rec.first;
  const bool overwritten = k + 1 < R && (nxt.flags & AM355_EDIT_UPDATE) && nxt.index == rec.index + count - 1;
  live = (rec.flags & AM355_EDIT_REMOVE) ? 0u : count - (overwritten ? 1u : 0u);
  return true;
}

// Pass 1, one thread per record: bytes[k] = bytes the record contributes, elems[k] = elements it leaves in the list, mark[k] = TM_STRING
// | TM_BOM; the elements that are no strings are summed into words[TW_NONSTR]. A record of values of >= 3 bytes is looked at value by
// value for the byte order mark: up to TEXT_BOM_INLINE values by its own thread, a longer one (a pasted run of three-byte characters) by
// the whole workgroup, 256 values per step.
__global__ __launch_bounds__(BLOCK) void kt_sizes(const am355_ir_edit* __restrict__ edit, uint32_t begin, uint32_t R, uint32_t n_values, const uint8_t* __restrict__ arena,
                                                  uint64_t arena_len, uint32_t* __restrict__ bytes, uint32_t* __restrict__ elems, uint8_t* __restrict__ mark,
                                                  uint32_t* __restrict__ words) {
  __shared__ uint32_t s_red[BLOCK / WAVE];
  __shared__ uint32_t s_n_long;
  __shared__ uint32_t s_owner[BLOCK], s_off[BLOCK], s_len[BLOCK], s_live[BLOCK];
  if (threadIdx.x == 0) s_n_long = 0;
  __syncthreads();
  const uint32_t k = gtid();
  uint32_t count = 0, live = 0, nbytes = 0, nonstr = 0, err = 0, boms = 0, len = 0;
  uint8_t m = 0;
  if (k < R) {
    const am355_ir_edit& rec = edit[begin + k];
    if (!text_live(edit, begin, R, k, n_values, count, live)) err |= TF_RANGE;
    const bool is_str = !(rec.flags & (AM355_EDIT_CHILD | AM355_EDIT_COUNTER | AM355_EDIT_REMOVE)) && (rec.val_tl & 15u) == 6u;
    if (!is_str) {
      nonstr = live;
    } else {
      len = rec.val_tl >> 4;
      if ((uint64_t)rec.val_off + (uint64_t)count * len > arena_len) {
        err |= TF_RANGE;   // (nothing of the record is read: bytes stay 0)
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
  if (k < R) { bytes[k] = nbytes; elems[k] = live; mark[k] = m; }
  const uint32_t wg_nonstr = block_sum_u32(nonstr, s_red);
  if (threadIdx.x == 0 && wg_nonstr) atomicAdd(&words[TW_NONSTR], wg_nonstr);
  if (err) atomicOr(&words[TW_FLAGS], err);
}

// Pass 3, parallel over the OUTPUT: a workgroup owns TEXT_WG_BYTES bytes, a thread TEXT_CHUNK of them (neighbouring threads write
// neighbouring 16-byte words; the binary search is a chain of dependent loads, so the more threads search side by side the better). It finds the record of its first byte by binary search over the scanned offsets (the last record
// that begins at or before it: the records of no bytes in between are passed over), and copies: one unaligned 16-byte load where the 16
// bytes lie in one unmarked record -- the case of a typed or pasted run --, byte by byte where records end inside them (a document typed
// character by character: sixteen records) or the record drops byte order marks. Always one aligned 16-byte store: the buffer is padded.
__global__ __launch_bounds__(BLOCK) void kt_gather(const am355_ir_edit* __restrict__ edit, uint32_t begin, uint32_t R, uint32_t n_values, const uint32_t* __restrict__ off,
                                                   const uint8_t* __restrict__ mark, uint32_t total, const uint8_t* __restrict__ arena, uint8_t* __restrict__ out) {
  {
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
      const U4 x = *(const U4*)(arena + edit[begin + k].val_off + (p - off[k]));
      w.x = x.x; w.y = x.y; w.z = x.z; w.w = x.w;
    } else {
      uint32_t rec_off = off[k], src = edit[begin + k].val_off;
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
            src = edit[begin + k].val_off;
            marked = (mark[k] & TM_BOM) != 0;
            cur_set = false;
          }
          uint32_t byte;
          if (!marked) {
            byte = arena[src + (q - rec_off)];
          } else {
            if (!cur_set) {
              uint32_t count;
              (void)text_live(edit, begin, R, k, n_values, count, cur_live);
              cur_len = edit[begin + k].val_tl >> 4;
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

int text_rank_of(am355_ctx* c, const uint8_t* actor, size_t len, uint32_t* rank) {
  // c->actors is the actor table by rank: lexicographic order of the raw ids
  const std::string want((const char*)actor, len);
  auto it = std::lower_bound(c->actors.begin(), c->actors.end(), want, [](const std::string& a, const std::string& b) {
    const size_t n = std::min(a.size(), b.size());
    const int d = n ? memcmp(a.data(), b.data(), n) : 0;
    return d ? d < 0 : a.size() < b.size();
  });
  if (it == c->actors.end() || *it != want) return 0;
  *rank = (uint32_t)(it - c->actors.begin());
  return 1;
}

std::string text_id(uint64_t ctr, const uint8_t* actor, size_t len) {
  static const char* d = "0123456789abcdef";
  std::string s = std::to_string((unsigned long long)ctr) + "@";
  for (size_t k = 0; k < len; k++) { s.push_back(d[actor[k] >> 4]); s.push_back(d[actor[k] & 15]); }
  return s;
}

int text_poll(am355_ctx* c) {   // (short copies and kernels: polled, not slept on -- fetch_ir_impl)
  hipError_t q;
  while ((q = hipStreamQuery(c->stream)) == hipErrorNotReady) {}
  if (q != hipSuccess) HIPCHK(c, q);
  return AM355_OK;
}

// The object a call names, for am355_object_text and the calls of am355_locate.hip: its index and its edit records [eb, ee). From the host's
// copy of the object table when it is the device's, else one launch over ir.obj (+ the launch that signals the four words; counted in
// *launches). The caller has checked the state and run ensure_ir_fresh.
int text_lookup(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, uint32_t& oi, uint32_t& eb, uint32_t& ee, uint64_t* launches) {
  hipStream_t st = c->stream;
  const uint32_t NO = c->counts.n_objects, NR = c->counts.n_erecs;
  const std::string id = text_id(obj_ctr, obj_actor, actor_len);
  if (obj_ctr == 0 && actor_len == 0) return fail(c, AM355_E_ARG, "not a Text object");   // (_root: a map)
  uint32_t rank = 0;
  if (obj_ctr > 0xffffffffull || !text_rank_of(c, obj_actor, actor_len, &rank)) return fail(c, AM355_E_ARG, "no such object: %s", id.c_str());

  // ---- the object: from the host's copy of the object table when it is the device's, else one launch over ir.obj ----
  if (!c->d_text.ensure(TW_WORDS * 4) || !c->h_text_sig.ensure((TW_WORDS + 1) * 4)) return fail(c, AM355_E_NOMEM, "allocation failed (text)");
  uint32_t* hw = c->h_text_sig.as<uint32_t>();
  volatile uint32_t* hseq = (volatile uint32_t*)(hw + TW_WORDS);
  if (c->text_seq == 0) *hseq = 0;
  uint32_t type = 0;
  oi = NONE32; eb = ee = 0;
  if (c->h_tables_current && c->hir.objects && c->hir.n_objects == NO) {
    for (uint32_t i = 1; i < NO; i++)
      if (c->hir.objects[i].id_ctr == (uint32_t)obj_ctr && c->hir.objects[i].id_actor == rank) {
        oi = i; type = c->hir.objects[i].type; eb = c->hir.objects[i].edit_begin; ee = c->hir.objects[i].edit_end;
        break;
      }
  } else if (NO > 1) {
    uint32_t* dw = c->d_text.as<uint32_t>();
    HIPCHK(c, hipMemsetAsync(dw, 0xff, 4 * 4, st));
    AM355_LAUNCH_INDEPENDENT(kt_find, dim3((NO + BLOCK - 1) / BLOCK), dim3(BLOCK), st, (const am355_ir_object*)c->ir.obj, NO, (uint32_t)obj_ctr, rank, dw);
    launch_signal_words(dw, 4, nullptr, 0, hw, hseq, ++c->text_seq, st);
    *launches += 2;
    if (!wait_host_signal(hseq, c->text_seq, st)) HIPCHK(c, hipMemcpy(hw, dw, 4 * 4, hipMemcpyDeviceToHost));
    oi = hw[TW_INDEX]; type = hw[TW_TYPE]; eb = hw[TW_BEGIN]; ee = hw[TW_END];
  }
  if (oi == NONE32) return fail(c, AM355_E_ARG, "no such object: %s", id.c_str());
  if (type != 4) return fail(c, AM355_E_ARG, "not a Text object");
  if (eb > ee || ee > NR) return fail(c, AM355_E_DEVICE, "internal: edit range [%u, %u) of object %u outside the %u records", eb, ee, oi, NR);
  return AM355_OK;
}

int object_text_impl(am355_ctx* c, uint64_t obj_ctr, const uint8_t* obj_actor, size_t actor_len, const uint8_t** utf8, size_t* len, am355_text_info* info) {
  if (!c) return AM355_E_ARG;
  if (!utf8 || !len || (!obj_actor && actor_len)) return fail(c, AM355_E_ARG, "am355_object_text: null argument");
  if (!c->replayed) return fail(c, AM355_E_STATE, "am355_object_text: a replayed state is needed");
  if (c->shard_world > 1) return fail(c, AM355_E_UNSUPPORTED, "am355_object_text on a sharded context");
  (void)hipSetDevice(c->device);
  { int frc = ensure_ir_fresh(c); if (frc) return frc; }   // (in-place list merges leave the edit tables stale: rebuilt once)
  hipStream_t st = c->stream;
  const uint32_t NV = c->counts.n_edits;
  uint32_t oi = NONE32, eb = 0, ee = 0;
  { int lrc = text_lookup(c, obj_ctr, obj_actor, actor_len, oi, eb, ee, &c->n_text_launches); if (lrc) return lrc; }
  uint32_t* hw = c->h_text_sig.as<uint32_t>();
  volatile uint32_t* hseq = (volatile uint32_t*)(hw + TW_WORDS);
  const uint32_t R = ee - eb;
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
    hipLaunchKernelGGL(kt_sizes, dim3((R + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, (const am355_ir_edit*)c->ir.edit, eb, R, NV, (const uint8_t*)c->mb.arena,
                       (uint64_t)c->raw.size(), d_off, d_elems, d_mark, dw);
    exclusive_scan2_u32(d_off, d_off, dw + TW_BYTES, d_elems, d_elems, dw + TW_ELEMS, R, d_ws, st);
    launch_signal_words(dw + TW_BYTES, 4, nullptr, 0, hw + TW_BYTES, hseq, ++c->text_seq, st);
    c->n_text_launches += 3;
    // the one wait of the read itself: the totals size the output
    if (!wait_host_signal(hseq, c->text_seq, st)) HIPCHK(c, hipMemcpy(hw + TW_BYTES, dw + TW_BYTES, 4 * 4, hipMemcpyDeviceToHost));
    const uint32_t tf = hw[TW_FLAGS];
    if (tf & TF_RANGE) return fail(c, AM355_E_DEVICE, "internal: an edit record of object %u names values outside the tables", oi);
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
      AM355_LAUNCH_INDEPENDENT(kt_gather, dim3(wgs), dim3(BLOCK), st, (const am355_ir_edit*)c->ir.edit, eb, R, NV, (const uint32_t*)d_off, (const uint8_t*)d_mark,
                               (uint32_t)total, (const uint8_t*)c->mb.arena, dst);
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
