// Device-wide primitives (see am355_prims.hip).
#pragma once
#include "am355_device.h"
#include "am355_canary.h"
#include <stddef.h>

namespace am355 {
// Ranges one launch of the two tables below takes (they are kernel arguments: the capacity is part of their layout).
constexpr uint32_t LAUNCH_RANGES = 8;
// Several word ranges filled with a value each in ONE launch (a memset per range costs a launch gap each). Ranges of <= 64 words
// are written by one thread in the order given (they may overlap: a later range wins); longer ones must not overlap.
// add(): false when the table is full (nothing is added).
struct FillRanges {
  uint32_t* p[LAUNCH_RANGES];
  uint32_t n_words[LAUNCH_RANGES];
  uint32_t value[LAUNCH_RANGES];
  uint32_t n = 0;
  bool add(void* q, size_t bytes, uint32_t v) {
    if (n == LAUNCH_RANGES) return false;
    p[n] = (uint32_t*)q; n_words[n] = (uint32_t)((bytes + 3) / 4); value[n] = v; n++;
    return true;
  }
};
void launch_fill_ranges(const FillRanges& f, hipStream_t st);
// Small host -> device copies as ONE launch: the kernel reads the (pinned, device-visible) sources over the link itself. A copy command
// costs the host ~5-8 us whatever its size; a call of Backend.applyChanges with a one-change batch has five of a few hundred bytes each.
struct CopyRanges {
  void* dst[LAUNCH_RANGES];
  const void* src[LAUNCH_RANGES];
  uint32_t bytes[LAUNCH_RANGES];
  uint32_t n = 0;
  bool add(void* d, const void* s, size_t b) {
    if (n == LAUNCH_RANGES) return false;
    dst[n] = d; src[n] = s; bytes[n] = (uint32_t)b; n++;
    return true;
  }
};
void launch_copy_ranges(const CopyRanges& r, hipStream_t st);
// Actor ranks rewritten where they are stored, x = table[x] for every x < n_old, in ONE launch (replay_resident: actors inserted into the
// sorted actor table renumber the ranks the kept state holds; a monotone renumbering, so no comparison between kept rows changes).
// A range is `count` rank words `stride` words apart: 1 = a dense column (16-byte loads and stores between its 16-byte boundaries), more =
// a field of a record table. guard != 0: the word `guard` words from the rank tells whether the rank means anything -- a record whose
// guard word equals guard_skip stays as it is (the _root object's id, an accumulator nothing was written to). Values >= n_old (NONE32 for
// _root, ...) stay bit-identical in every range. add(): false when the table is full (nothing is added).
constexpr uint32_t REMAP_WG_ROWS = 1024;    // ranks of a dense column one workgroup rewrites per step of its grid-stride loop (4 per thread)
constexpr uint32_t REMAP_LDS_RANKS = 4096;  // the table is staged in LDS up to this many old ranks (16 KB), read through L2 beyond
struct RemapRanges {
  uint32_t* p[LAUNCH_RANGES];
  uint32_t count[LAUNCH_RANGES];
  uint32_t stride[LAUNCH_RANGES];
  int32_t guard[LAUNCH_RANGES];
  uint32_t guard_skip[LAUNCH_RANGES];
  uint32_t n = 0;
  bool add(uint32_t* first_rank, size_t n_ranks, uint32_t stride_words = 1, int32_t guard_at = 0, uint32_t skip = 0) {
    if (n == LAUNCH_RANGES || n_ranks > 0xffffffffu || !stride_words) return false;
    if (!n_ranks) return true;
    p[n] = first_rank; count[n] = (uint32_t)n_ranks; stride[n] = stride_words; guard[n] = guard_at; guard_skip[n] = skip; n++;
    return true;
  }
};
// d_table: [n_old] device words, table[old rank] = new rank
void launch_remap_ranks(const RemapRanges& r, const uint32_t* d_table, uint32_t n_old, hipStream_t st);
// Result words of a phase into pinned host memory, then the sequence number (signal_host, am355_device.h), as a one-thread launch of its
// own behind the phase: for phases that end in a library scan or in one of several kernels. Two source ranges, a then b (n_b may be 0).
void launch_signal_words(const uint32_t* src_a, uint32_t n_a, const uint32_t* src_b, uint32_t n_b, uint32_t* host_words, volatile uint32_t* host_seq, uint32_t seq,
                         hipStream_t st);
size_t scan_workspace_bytes(uint32_t n);
uint32_t scan_single_limit();   // arrays of up to this many elements are scanned by one workgroup in one launch
// out[i] = sum(in[0..i)); in == out allowed. *d_total (device, optional) receives the grand total.
void exclusive_scan_u32(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* d_total, void* ws, hipStream_t st);
// out[i] = number of bytes in [0, i) with bit 7 clear (LEB128 terminators), i = 0 .. L: the scan of a flag array that is never stored
void exclusive_scan_terminators(const uint8_t* bytes, uint32_t L, uint32_t* out, uint32_t* d_total, void* ws, hipStream_t st);
// two scans over the same range in one pass (same workspace size); in == out allowed, totals optional
void exclusive_scan2_u32(const uint32_t* in_a, uint32_t* out_a, uint32_t* d_total_a, const uint32_t* in_b, uint32_t* out_b, uint32_t* d_total_b, uint32_t n,
                         void* ws, hipStream_t st);
// *d_out = max(*d_out, max(v[0..n)))
void max_u32(const uint32_t* v, uint32_t n, uint32_t* d_out, hipStream_t st);
size_t sort_workspace_bytes(uint32_t n);
// Stable LSD sort of (key, value) pairs, ascending, by WHOLE 8-bit digits from begin_bit up: ceil((end_bit - begin_bit) / 8) passes
// (none when end_bit <= begin_bit: the pairs stay where they are), pass k by bits [begin_bit + 8 k, begin_bit + 8 k + 8) (a digit that
// reaches past bit 63 is filled with zeros). So every key bit in [begin_bit, begin_bit + 8 * passes) takes part -- also the ones between
// end_bit and the top of the last digit, which the CONTRACT wants zero in every key (or equal in all of them): callers build their keys
// from fields that add up to end_bit bits and leave everything above zero, or pass whole bytes (order_map_emissions). Bits below begin_bit
// and above the last digit are carried along and never looked at. Pairs whose looked-at bits are equal keep their input order.
// Returns where the result lies: 0 = (keys_a, vals_a), 1 = (keys_b, vals_b) -- the parity of the number of passes (0 when n == 0: nothing is launched);
// the other pair of buffers holds the state before the last pass.
// first_hist_done: the caller's own kernel (the one that produced keys_a) has already left the histogram of the FIRST digit (bits
// [begin_bit, begin_bit + 8)) in sort_first_table(ws), laid out [digit x sort_tiles(n) + tile] over tiles of SORT_TILE_ELEMS elements --
// only for sorts with sort_is_fused(n)
int radix_sort_pairs(uint64_t* keys_a, uint32_t* vals_a, uint64_t* keys_b, uint32_t* vals_b, uint32_t n, int begin_bit, int end_bit,
                     void* ws, hipStream_t st, bool first_hist_done = false);
constexpr uint32_t SORT_TILE_ELEMS = 2048;
uint32_t sort_tiles(uint32_t n);
bool sort_is_fused(uint32_t n);
uint32_t* sort_first_table(void* ws);
// Forward chain marking: next[i] > i, or >= n (NONE32) at the end of a chain. mark[] holds the start nodes on entry and
// is nonzero on every node reachable from a start on return (values already nonzero are kept). `work` needs
// chain_work_bytes(n) bytes.
size_t chain_work_bytes(uint32_t n);
void chain_mark(const uint32_t* next, uint32_t n, uint32_t* mark, void* work, hipStream_t st);
}  // namespace am355
