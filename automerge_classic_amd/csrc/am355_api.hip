// C ABI of the replay engine (include/am355.h): context, staging, host-side causal scheduler, orchestration of
// the device stages, patch-IR download.
//
// Host-side logic restated from the reference (paths relative to the reference tree):
//   inflate of DEFLATEd changes    backend/columnar.js:813-823 inflateChange (zlib raw inflate)
//   causal scheduling              backend/new.js:1550-1597 applyChanges, :1822-1841 retry loop
//   actor table                    backend/new.js:1434-1451 getActorTable (first-applied order; the engine
//                                  additionally ranks actors lexicographically for numeric op-id comparison)
//   envelope                       backend/new.js:1870-1873, 2064-2067 (maxOp, clock, deps, pendingChanges)
#include "am355_ctx.h"
#include "am355_scan.h"
#include "am355_textrec.h"

// the context's host threads, streams, events and signal words; false: something could not be made (the caller deletes the context,
// which destroys what was)
static bool ctx_init(am355_ctx* c) {
  {
    unsigned hw = std::thread::hardware_concurrency();
    const char* env = getenv("AM355_HOST_THREADS");
    unsigned want = env && atoi(env) > 0 ? (unsigned)atoi(env) : std::min(hw ? hw : 4u, 64u);  // (measured on a 2 x 64-core host: inflating 4 k changes scales to ~64 threads; jobs wake only the workers they need)
    c->pool.reset(new HostPool(want > 1 ? want - 1 : 0));  // (the calling thread works too)
  }
  // the decode/merge stream outranks the hash stream: their small grids would otherwise share SIMDs and the
  // ALU-dense SHA-256 waves slow the latency-bound parse/decode waves down
  int prio_low = 0, prio_high = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
  auto make_stream = [](Stream& s, int prio) { return hipStreamCreateWithPriority(&s.h, hipStreamNonBlocking, prio) == hipSuccess; };
  if (!make_stream(c->stream, prio_high)) return false;
  {
    // The hash stream (one lane per change: ~65 waves of dependent SHA-256 rounds for 4 k changes) gets its own few compute
    // units when AM355_HASH_CUS=n asks for it (hipExtStreamCreateWithCUMask: its waves then never share a SIMD with the
    // latency-bound kernels of the critical path); by default it is an ordinary low-priority stream.
    const char* env = getenv("AM355_HASH_CUS");
    int want = env ? atoi(env) : 0;
    bool made = false;
    if (want > 0) {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > want) {
        int n_cu = prop.multiProcessorCount;
        std::vector<uint32_t> mask((size_t)(n_cu + 31) / 32, 0u);
        for (int k = 0; k < want; k++) { int cu = n_cu - 1 - k; mask[(size_t)cu / 32] |= 1u << (cu % 32); }
        made = hipExtStreamCreateWithCUMask(&c->stream2.h, (uint32_t)mask.size(), mask.data()) == hipSuccess;
      }
    }
    if (!made && !make_stream(c->stream2, prio_low)) return false;
  }
  if (!make_stream(c->stream3, prio_high) || !make_stream(c->stream4, prio_high)) return false;
  for (Event* e : {&c->ev_fork, &c->ev_join, &c->ev[0], &c->ev[1], &c->ev[2], &c->ev[3], &c->ev[4], &c->ev[5], &c->ev[6], &c->ev[7], &c->ev_parse, &c->ev_b0, &c->ev_b1,
                   &c->ev_counts, &c->ev_runs, &c->ev_s1, &c->ev_plan, &c->ev_tables, &c->ev_fills, &c->ev_sched})
    if (hipEventCreate(&e->h) != hipSuccess) return false;
  if (!c->h_sig.ensure(sizeof(HostSignals))) return false;
  memset(c->h_sig.p, 0, sizeof(HostSignals));
  if (const char* e = getenv("AM355_PHASE_EVENTS")) c->phase_events = strcmp(e, "0") != 0;
  return true;
}

extern "C" am355_ctx* am355_create(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return nullptr;
  // every replay has a few host round trips of some microseconds each: wait for them actively (refused, harmlessly, when the
  // host process has already initialised the device with other flags)
  (void)hipSetDeviceFlags(hipDeviceScheduleSpin);
  if (hipSetDevice(device) != hipSuccess) return nullptr;
  am355_ctx* c = new am355_ctx();
  c->device = device;
  if (!ctx_init(c)) { delete c; return nullptr; }
  return c;
}

// Everything that may still touch a member comes to rest first: the lane's job captures the context, the checksum thread reads
// doc_bytes, the streams' commands read and write the buffers. (The host pool works inside calls only.) Nothing is running after
// that, so the order in which the members then go -- the reverse of their declaration -- does not matter: buffers, streams and events
// release themselves, the threads of `pool`, `lane` and `doc_sum` are idle and joined by their owners.
am355_ctx::~am355_ctx() {
  (void)hipSetDevice(device);   // (canary_forget asks for the current device; another context may have changed it)
  if (lane) lane->wait();
  (void)doc_sum.wait();
  for (const Stream* s : {&stream, &stream2, &stream3, &stream4})
    if (s->h) (void)hipStreamSynchronize(s->h);   // (null: am355_create failed before it was made)
  if (shard_comm) (void)am355_shard_finalize(this);   // (ncclCommDestroy)
}

extern "C" void am355_destroy(am355_ctx* c) {
  delete c;   // (of a null pointer: nothing)
}

extern "C" const char* am355_last_error(const am355_ctx* c) { return c ? c->err.c_str() : "no context (no GPU?)"; }
extern "C" uint32_t am355_flags(const am355_ctx* c) { return c ? c->flags : 0; }

extern "C" int am355_set_phase_events(am355_ctx* c, int on) {
  if (!c) return AM355_E_ARG;
  c->phase_events = on != 0;
  return AM355_OK;
}

extern "C" int am355_get_stats(const am355_ctx* c, am355_stats* out) {
  if (!c || !out) return AM355_E_ARG;
  *out = c->stats;
  return AM355_OK;
}

extern "C" int am355_get_hashes(const am355_ctx* c, uint8_t* out) {
  if (!c || !out) return AM355_E_ARG;
  if (!c->replayed || !c->h_hashes.p || c->is_document) return AM355_E_STATE;  // a document stores no per-change hashes
  memcpy(out, c->h_hashes.p, 32 * (size_t)c->n_changes);
  return AM355_OK;
}

extern "C" int am355_arena_epoch(const am355_ctx* c, uint64_t* epoch) {
  if (!c || !epoch) return AM355_E_ARG;
  *epoch = c->arena_epoch;
  return AM355_OK;
}

extern "C" int am355_get_hashes_range(const am355_ctx* c, uint32_t first, uint32_t count, uint8_t* out) {
  if (!c || (!out && count)) return AM355_E_ARG;
  if (!c->replayed || !c->h_hashes.p || c->is_document) return AM355_E_STATE;
  if (first > c->n_changes || count > c->n_changes - first) return AM355_E_ARG;
  if (count) memcpy(out, (const uint8_t*)c->h_hashes.p + 32 * (size_t)first, 32 * (size_t)count);
  return AM355_OK;
}

extern "C" int am355_applied_in_input_order(const am355_ctx* c, int* yes) {
  if (!c || !yes) return AM355_E_ARG;
  if (!c->replayed || c->is_document) return AM355_E_STATE;
  bool ok = c->pending_change.empty() && c->n_pending == 0 && c->applied_change.size() == c->n_changes;
  for (uint32_t i = 0; ok && i < c->n_changes; i++) ok = c->applied_change[i] == i;
  *yes = ok ? 1 : 0;
  return AM355_OK;
}

extern "C" int am355_resident_counters(const am355_ctx* c, uint64_t out[3]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_resident_calls;
  out[1] = c->n_resident_fallbacks;
  out[2] = c->n_resorder_calls;
  return AM355_OK;
}

extern "C" int am355_resident_maps_only_calls(const am355_ctx* c, uint64_t* out) {
  if (!c || !out) return AM355_E_ARG;
  *out = c->n_maps_only_calls;
  return AM355_OK;
}

extern "C" int am355_set_resident_new_actors(am355_ctx* c, int on) {
  if (!c) return AM355_E_ARG;
  c->resident_new_actors = on != 0;
  return AM355_OK;
}

extern "C" int am355_resident_new_actor_calls(const am355_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_new_actor_calls;
  out[1] = c->n_rank_rewrites;
  return AM355_OK;
}

extern "C" int am355_set_resident_map_merge(am355_ctx* c, int on) {
  if (!c) return AM355_E_ARG;
  c->resident_map_merge = on != 0;
  return AM355_OK;
}

extern "C" int am355_resident_map_merge_calls(const am355_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_map_merge_calls;
  out[1] = c->n_map_merge_declined;
  return AM355_OK;
}

extern "C" int am355_set_resident_new_objects(am355_ctx* c, int on) {
  if (!c) return AM355_E_ARG;
  c->resident_new_objects = on != 0;
  return AM355_OK;
}

extern "C" int am355_resident_new_object_calls(const am355_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_new_object_calls;
  out[1] = c->n_new_object_declined;
  return AM355_OK;
}

extern "C" int am355_set_resident_counters(am355_ctx* c, int on) {
  if (!c) return AM355_E_ARG;
  c->resident_counters = on != 0;
  return AM355_OK;
}

extern "C" int am355_set_local_small(am355_ctx* c, int on) {
  if (!c) return AM355_E_ARG;
  c->local_small = on != 0;
  return AM355_OK;
}

extern "C" int am355_local_small_calls(const am355_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_local_small;
  out[1] = c->n_local_small_bulk;
  return AM355_OK;
}

extern "C" int am355_resident_counter_calls(const am355_ctx* c, uint64_t out[2]) {
  if (!c || !out) return AM355_E_ARG;
  out[0] = c->n_counter_calls;
  out[1] = c->n_counter_declined;
  return AM355_OK;
}

extern "C" int am355_get_raw(const am355_ctx* c, const uint8_t** arena, const uint64_t** offsets, uint32_t* n) {
  if (!c || !c->staged) return AM355_E_STATE;
  if (arena) *arena = c->raw.data();
  if (offsets) *offsets = c->raw_off.data();
  if (n) *n = c->n_changes;
  return AM355_OK;
}

// ---------------------------------------------------------------------------------------------------------
// IR download + JSON
// ---------------------------------------------------------------------------------------------------------
extern "C" int am355_get_applied(const am355_ctx* c, uint32_t* out, uint32_t* n_applied) {
  if (!c || !n_applied) return AM355_E_ARG;
  if (!c->replayed || c->is_document) return AM355_E_STATE;
  *n_applied = (uint32_t)c->applied_change.size();
  if (out) memcpy(out, c->applied_change.data(), 4 * c->applied_change.size());
  return AM355_OK;
}

// with_edits = false (am355_apply_changes): the object and map tables only -- the edit records of a text document are megabytes and
// setupPatches looks at them only when a touched object hangs in a list (c->hir.edits stays null; a later full fetch copies all three)
extern "C" int am355_test_sort(am355_ctx* c, uint64_t* keys, uint32_t* vals, uint32_t n, int key_bits) {
  if (!c) return AM355_E_ARG;
  (void)hipSetDevice(c->device);
  DevBuf ka, kb, va, vb, ws;
  if (!ka.ensure(8 * (size_t)n + 8) || !kb.ensure(8 * (size_t)n + 8) || !va.ensure(4 * (size_t)n + 4) || !vb.ensure(4 * (size_t)n + 4) || !ws.ensure(sort_workspace_bytes(n)))
    return fail(c, AM355_E_NOMEM, "alloc");
  hipStream_t st = c->stream;
  (void)hipMemcpyAsync(ka.p, keys, 8 * (size_t)n, hipMemcpyHostToDevice, st);
  (void)hipMemcpyAsync(va.p, vals, 4 * (size_t)n, hipMemcpyHostToDevice, st);
  int res = radix_sort_pairs(ka.as<uint64_t>(), va.as<uint32_t>(), kb.as<uint64_t>(), vb.as<uint32_t>(), n, 0, key_bits, ws.p, st);
  (void)hipMemcpyAsync(keys, res ? kb.p : ka.p, 8 * (size_t)n, hipMemcpyDeviceToHost, st);
  (void)hipMemcpyAsync(vals, res ? vb.p : va.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st);
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipGetLastError());
  return AM355_OK;
}

extern "C" int am355_test_scan(am355_ctx* c, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* total) {
  if (!c) return AM355_E_ARG;
  (void)hipSetDevice(c->device);
  DevBuf di, dt, ws;
  if (!di.ensure(4 * (size_t)n + 4) || !dt.ensure(4) || !ws.ensure(scan_workspace_bytes(n))) return fail(c, AM355_E_NOMEM, "alloc");
  hipStream_t st = c->stream;
  (void)hipMemcpyAsync(di.p, in, 4 * (size_t)n, hipMemcpyHostToDevice, st);
  exclusive_scan_u32(di.as<uint32_t>(), di.as<uint32_t>(), n, dt.as<uint32_t>(), ws.p, st);
  (void)hipMemcpyAsync(out, di.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st);
  (void)hipMemcpyAsync(total, dt.p, 4, hipMemcpyDeviceToHost, st);
  HIPCHK(c, hipStreamSynchronize(st));
  return AM355_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The device primitives of am355_prims.h and the workgroup / carried scans of am355_scan.h, each driven by itself
// (tests/test_primitives.py). A hook uploads the caller's buffer images WHOLE, hands the primitive a pointer some words (bytes) into
// them, and downloads them whole: the caller sees what was written around a range as well as in it. Offsets and ranges that would
// leave an image are refused with AM355_E_ARG before anything is launched.
// ---------------------------------------------------------------------------------------------------------
namespace {
// device image of a host buffer, 16-byte aligned whatever the allocator gives
struct TestImage {
  DevBuf d;
  uint8_t* p = nullptr;
  size_t bytes = 0;
  bool up(const void* host, size_t n, hipStream_t st) {
    if (!d.ensure(n + 16)) return false;
    p = (uint8_t*)(((uintptr_t)d.p + 15) & ~(uintptr_t)15);
    bytes = n;
    if (n) (void)hipMemcpyAsync(p, host, n, hipMemcpyHostToDevice, st);
    return true;
  }
  void down(void* host, hipStream_t st) const {
    if (bytes) (void)hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, st);
  }
  uint32_t* words(size_t off = 0) const { return (uint32_t*)p + off; }
};
int test_finish(am355_ctx* c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  return AM355_OK;
}

// carried scan: the producer / consumer pair of the replay kernels, one value per thread (am355_scan.h)
__global__ __launch_bounds__(BLOCK) void k_test_carry_produce(const uint32_t* __restrict__ v, uint32_t n, CarryScan cs) {
  __shared__ uint32_t s[BLOCK / WAVE];
  const uint32_t i = gtid();
  (void)carry_publish(cs, i < n ? v[i] : 0u, s);
}
// out: the exclusive prefix over the grid (carry_prefix); out_wg / wg_total: over the workgroup alone (block_exclusive_scan_u32)
__global__ __launch_bounds__(BLOCK) void k_test_carry_consume(const uint32_t* __restrict__ v, uint32_t n, CarryScan cs, uint32_t* __restrict__ out,
                                                              uint32_t* __restrict__ out_wg, uint32_t* __restrict__ wg_total) {
  __shared__ uint32_t s[BLOCK / WAVE];
  const uint32_t i = gtid();
  const uint32_t x = i < n ? v[i] : 0u;
  uint32_t total;
  const uint32_t in_wg = block_exclusive_scan_u32(x, s, &total);
  const uint32_t pre = carry_prefix(cs, x, s);
  if (i < n) { out[i] = pre; out_wg[i] = in_wg; }
  if (threadIdx.x == 0) wg_total[blockIdx.x] = total;
}
}  // namespace

extern "C" int am355_test_scan_at(am355_ctx* c, uint32_t* in_buf, uint32_t in_words, uint32_t in_off, uint32_t* out_buf, uint32_t out_words, uint32_t out_off, uint32_t n,
                                  uint32_t* total) {
  if (!c || !in_buf) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    const bool in_place = !out_buf;
    if (in_off > 3 || out_off > 3 || (size_t)in_off + n > in_words || (in_place ? out_off != in_off : (size_t)out_off + n > out_words))
      return fail(c, AM355_E_ARG, "am355_test_scan_at: the range leaves its buffer");
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage di, dout, dt;
    DevBuf ws;
    uint32_t none = 0;
    if (!di.up(in_buf, 4 * (size_t)in_words, st) || !dout.up(out_buf, in_place ? 0 : 4 * (size_t)out_words, st) || !dt.up(total ? total : &none, 4, st) ||
        !ws.ensure(scan_workspace_bytes(n)))
      return fail(c, AM355_E_NOMEM, "alloc");
    exclusive_scan_u32(di.words(in_off), in_place ? di.words(in_off) : dout.words(out_off), n, total ? dt.words() : nullptr, ws.p, st);
    di.down(in_buf, st);
    dout.down(out_buf, st);
    if (total) dt.down(total, st);
    return test_finish(c);
  });
}

extern "C" int am355_test_scan2(am355_ctx* c, uint32_t* in_a, uint32_t* in_b, uint32_t in_words, uint32_t in_off, uint32_t* out_a, uint32_t* out_b, uint32_t out_words,
                                uint32_t out_off, uint32_t n, uint32_t* total_a, uint32_t* total_b) {
  if (!c || !in_a || !in_b || !out_a != !out_b) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    const bool in_place = !out_a;
    if (in_off > 3 || out_off > 3 || (size_t)in_off + n > in_words || (in_place ? out_off != in_off : (size_t)out_off + n > out_words))
      return fail(c, AM355_E_ARG, "am355_test_scan2: the range leaves its buffer");
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage da, db, oa, ob, dt;
    DevBuf ws;
    uint32_t t2[2] = {total_a ? *total_a : 0u, total_b ? *total_b : 0u};
    const size_t ob_bytes = in_place ? 0 : 4 * (size_t)out_words;
    if (!da.up(in_a, 4 * (size_t)in_words, st) || !db.up(in_b, 4 * (size_t)in_words, st) || !oa.up(out_a, ob_bytes, st) || !ob.up(out_b, ob_bytes, st) || !dt.up(t2, 8, st) ||
        !ws.ensure(scan_workspace_bytes(n)))
      return fail(c, AM355_E_NOMEM, "alloc");
    exclusive_scan2_u32(da.words(in_off), in_place ? da.words(in_off) : oa.words(out_off), total_a ? dt.words(0) : nullptr, db.words(in_off),
                        in_place ? db.words(in_off) : ob.words(out_off), total_b ? dt.words(1) : nullptr, n, ws.p, st);
    da.down(in_a, st);
    db.down(in_b, st);
    oa.down(out_a, st);
    ob.down(out_b, st);
    dt.down(t2, st);
    int rc = test_finish(c);
    if (rc != AM355_OK) return rc;
    if (total_a) *total_a = t2[0];
    if (total_b) *total_b = t2[1];
    return AM355_OK;
  });
}

extern "C" int am355_test_scan_terminators(am355_ctx* c, const uint8_t* bytes_buf, size_t bytes_len, uint32_t byte_off, uint32_t L, uint32_t* out_buf, uint32_t out_words,
                                           uint32_t out_off, uint32_t* total) {
  if (!c || !bytes_buf || !out_buf) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    if (byte_off > 7 || out_off > 3 || L == 0xffffffffu || (size_t)byte_off + L > bytes_len || (size_t)out_off + L + 1 > out_words)
      return fail(c, AM355_E_ARG, "am355_test_scan_terminators: the range leaves its buffer");
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage db, dout, dt;
    DevBuf ws;
    uint32_t none = 0;
    if (!db.up(bytes_buf, bytes_len, st) || !dout.up(out_buf, 4 * (size_t)out_words, st) || !dt.up(total ? total : &none, 4, st) || !ws.ensure(scan_workspace_bytes(L + 1)))
      return fail(c, AM355_E_NOMEM, "alloc");
    exclusive_scan_terminators(db.p + byte_off, L, dout.words(out_off), total ? dt.words() : nullptr, ws.p, st);
    dout.down(out_buf, st);
    if (total) dt.down(total, st);
    return test_finish(c);
  });
}

// *inout: what *d_out holds before the call, and after it
extern "C" int am355_test_max(am355_ctx* c, const uint32_t* v, uint32_t n, uint32_t* inout) {
  if (!c || (!v && n) || !inout) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage dv, dm;
    if (!dv.up(v, 4 * (size_t)n, st) || !dm.up(inout, 4, st)) return fail(c, AM355_E_NOMEM, "alloc");
    max_u32(dv.words(), n, dm.words(), st);
    dm.down(inout, st);
    return test_finish(c);
  });
}

// first_table: null, or the histogram of the first digit as the caller computed it ([digit x sort_tiles(n) + tile], am355_prims.h): uploaded
// to sort_first_table(ws) and the sort called with first_hist_done. *result_buffer: what radix_sort_pairs returned; keys / vals come
// back from that buffer.
extern "C" int am355_test_sort_bits(am355_ctx* c, uint64_t* keys, uint32_t* vals, uint32_t n, int begin_bit, int end_bit, const uint32_t* first_table, int* result_buffer) {
  if (!c || ((!keys || !vals) && n) || !result_buffer) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    if (begin_bit < 0 || end_bit > 64 || begin_bit > end_bit) return fail(c, AM355_E_ARG, "am355_test_sort_bits: bits [%d, %d)", begin_bit, end_bit);
    if (first_table && !sort_is_fused(n)) return fail(c, AM355_E_ARG, "am355_test_sort_bits: first_hist_done is for fused sorts only (%u elements are %u tiles)", n, sort_tiles(n));
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage ka, va;
    DevBuf kb, vb, ws;
    if (!ka.up(keys, 8 * (size_t)n, st) || !kb.ensure(8 * (size_t)n + 8) || !va.up(vals, 4 * (size_t)n, st) || !vb.ensure(4 * (size_t)n + 4) || !ws.ensure(sort_workspace_bytes(n)))
      return fail(c, AM355_E_NOMEM, "alloc");
    if (first_table && n) (void)hipMemcpyAsync(sort_first_table(ws.p), first_table, 4 * (size_t)256 * sort_tiles(n), hipMemcpyHostToDevice, st);
    const int res = radix_sort_pairs((uint64_t*)ka.p, va.words(), kb.as<uint64_t>(), vb.as<uint32_t>(), n, begin_bit, end_bit, ws.p, st, first_table != nullptr);
    if (n) {
      (void)hipMemcpyAsync(keys, res ? kb.p : (void*)ka.p, 8 * (size_t)n, hipMemcpyDeviceToHost, st);
      (void)hipMemcpyAsync(vals, res ? vb.p : (void*)va.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st);
    }
    *result_buffer = res;
    return test_finish(c);
  });
}

// mark: [mark_words >= n] words, the first n are the marks
extern "C" int am355_test_chain_mark(am355_ctx* c, const uint32_t* next, uint32_t* mark, uint32_t mark_words, uint32_t n) {
  if (!c || ((!next || !mark) && n) || mark_words < n) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage dn, dm;
    DevBuf work;
    if (!dn.up(next, 4 * (size_t)n, st) || !dm.up(mark, 4 * (size_t)mark_words, st) || !work.ensure(chain_work_bytes(n))) return fail(c, AM355_E_NOMEM, "alloc");
    chain_mark(dn.words(), n, dm.words(), work.p, st);
    dm.down(mark, st);
    return test_finish(c);
  });
}

// ranges: n_ranges x {first word (an offset into buf, base_off is added), count, stride, guard (int32), guard_skip}. *n_added: the ranges
// the table held at the launch. AM355_E_ARG: RemapRanges::add() refused one (nothing is launched then).
extern "C" int am355_test_remap(am355_ctx* c, uint32_t* buf, uint32_t words, uint32_t base_off, const uint32_t* ranges, uint32_t n_ranges, const uint32_t* table,
                                uint32_t n_old, uint32_t* n_added) {
  if (!c || !buf || (!ranges && n_ranges) || (!table && n_old)) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage db, dt;
    if (!db.up(buf, 4 * (size_t)words, st) || !dt.up(table, 4 * (size_t)n_old, st)) return fail(c, AM355_E_NOMEM, "alloc");
    RemapRanges r;
    for (uint32_t k = 0; k < n_ranges; k++) {
      const uint32_t* q = ranges + 5 * (size_t)k;
      const int64_t first = (int64_t)base_off + q[0], count = q[1], stride = q[2], guard = (int32_t)q[3];
      if (count && stride) {
        const int64_t last = first + (count - 1) * stride;
        if (base_off > 3 || last >= (int64_t)words || first + guard < 0 || last + guard >= (int64_t)words || (guard && (guard <= -stride || guard >= stride)))
          return fail(c, AM355_E_ARG, "am355_test_remap: range %u leaves the buffer (or its guard the record)", k);
      }
      if (!r.add(db.words((size_t)first), (size_t)count, (uint32_t)stride, (int32_t)guard, q[4])) return fail(c, AM355_E_ARG, "am355_test_remap: add() refused range %u", k);
    }
    if (n_added) *n_added = r.n;
    launch_remap_ranks(r, dt.words(), n_old, st);
    db.down(buf, st);
    return test_finish(c);
  });
}

// ranges: n_ranges x {first word (+ base_off), BYTES, value}
extern "C" int am355_test_fill(am355_ctx* c, uint32_t* buf, uint32_t words, uint32_t base_off, const uint32_t* ranges, uint32_t n_ranges, uint32_t* n_added) {
  if (!c || !buf || (!ranges && n_ranges)) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage db;
    if (!db.up(buf, 4 * (size_t)words, st)) return fail(c, AM355_E_NOMEM, "alloc");
    FillRanges f;
    for (uint32_t k = 0; k < n_ranges; k++) {
      const uint32_t* q = ranges + 3 * (size_t)k;
      const size_t first = (size_t)base_off + q[0];
      if (base_off > 3 || first + ((size_t)q[1] + 3) / 4 > words) return fail(c, AM355_E_ARG, "am355_test_fill: range %u leaves the buffer", k);
      if (!f.add(db.words(first), q[1], q[2])) return fail(c, AM355_E_ARG, "am355_test_fill: add() refused range %u", k);
    }
    if (n_added) *n_added = f.n;
    launch_fill_ranges(f, st);
    db.down(buf, st);
    return test_finish(c);
  });
}

// ranges: n_ranges x {byte offset into dst, byte offset into src, bytes}. src_pinned: the source lies in pinned host memory and the kernel
// reads it over the link (the product's case); else in device memory.
extern "C" int am355_test_copy(am355_ctx* c, uint8_t* dst, size_t dst_bytes, const uint8_t* src, size_t src_bytes, int src_pinned, const uint32_t* ranges, uint32_t n_ranges,
                               uint32_t* n_added) {
  if (!c || !dst || !src || (!ranges && n_ranges)) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage dd, ds;
    HostBuf hs;
    const uint8_t* s0;
    if (!dd.up(dst, dst_bytes, st)) return fail(c, AM355_E_NOMEM, "alloc");
    if (src_pinned) {
      if (!hs.ensure(src_bytes + 16)) return fail(c, AM355_E_NOMEM, "alloc");
      uint8_t* h = (uint8_t*)(((uintptr_t)hs.p + 15) & ~(uintptr_t)15);
      memcpy(h, src, src_bytes);
      s0 = h;
    } else {
      if (!ds.up(src, src_bytes, st)) return fail(c, AM355_E_NOMEM, "alloc");
      s0 = ds.p;
    }
    CopyRanges r;
    for (uint32_t k = 0; k < n_ranges; k++) {
      const uint32_t* q = ranges + 3 * (size_t)k;
      if ((size_t)q[0] + q[2] > dst_bytes || (size_t)q[1] + q[2] > src_bytes) return fail(c, AM355_E_ARG, "am355_test_copy: range %u leaves its buffer", k);
      if (!r.add(dd.p + q[0], s0 + q[1], q[2])) return fail(c, AM355_E_ARG, "am355_test_copy: add() refused range %u", k);
    }
    if (n_added) *n_added = r.n;
    launch_copy_ranges(r, st);
    dd.down(dst, st);
    return test_finish(c);   // (the pinned source lives until here: the kernel has run)
  });
}

// host_words: [host_words_n >= n_a + n_b] words as pinned memory holds them before the launch, and after it; *seq_word likewise
extern "C" int am355_test_signal_words(am355_ctx* c, const uint32_t* a, uint32_t n_a, const uint32_t* b, uint32_t n_b, uint32_t seq, uint32_t* host_words,
                                       uint32_t host_words_n, uint32_t* seq_word) {
  if (!c || (!a && n_a) || (!b && n_b) || !host_words || !seq_word || (size_t)n_a + n_b > host_words_n) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage da, db;
    HostBuf h;
    if (!da.up(a, 4 * (size_t)n_a, st) || !db.up(b, 4 * (size_t)n_b, st) || !h.ensure(4 * ((size_t)host_words_n + 1))) return fail(c, AM355_E_NOMEM, "alloc");
    uint32_t* hw = h.as<uint32_t>();
    memcpy(hw, host_words, 4 * (size_t)host_words_n);
    hw[host_words_n] = *seq_word;
    launch_signal_words(da.words(), n_a, db.words(), n_b, hw, (volatile uint32_t*)(hw + host_words_n), seq, st);
    int rc = test_finish(c);
    if (rc != AM355_OK) return rc;
    memcpy(host_words, hw, 4 * (size_t)host_words_n);
    *seq_word = hw[host_words_n];
    return AM355_OK;
  });
}

// out: carry_prefix of v over the grid; out_wg / wg_total ([(n + 255) / 256]): block_exclusive_scan_u32 of v over each workgroup and its sum
extern "C" int am355_test_carried_scan(am355_ctx* c, const uint32_t* v, uint32_t n, uint32_t* out, uint32_t* out_wg, uint32_t* wg_total) {
  if (!c || !v || !out || !out_wg || !wg_total || !n || n > 0xffffff00u) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    const uint32_t wgs = (n + BLOCK - 1) / BLOCK;
    const size_t group_words = ((size_t)(wgs >> CARRY_GROUP_SHIFT) + 1) * CARRY_GROUP_STRIDE;
    TestImage dv;
    DevBuf d_out, d_wg, d_tot, d_carry;
    if (!dv.up(v, 4 * (size_t)n, st) || !d_out.ensure(4 * (size_t)n) || !d_wg.ensure(4 * (size_t)n) || !d_tot.ensure(4 * (size_t)wgs) ||
        !d_carry.ensure(4 * (wgs + group_words)))
      return fail(c, AM355_E_NOMEM, "alloc");
    CarryScan cs;
    cs.wg_sum = d_carry.as<uint32_t>();
    cs.group_sum = cs.wg_sum + wgs;
    (void)hipMemsetAsync(cs.group_sum, 0, 4 * group_words, st);
    hipLaunchKernelGGL(k_test_carry_produce, dim3(wgs), dim3(BLOCK), 0, st, (const uint32_t*)dv.words(), n, cs);
    hipLaunchKernelGGL(k_test_carry_consume, dim3(wgs), dim3(BLOCK), 0, st, (const uint32_t*)dv.words(), n, cs, d_out.as<uint32_t>(), d_wg.as<uint32_t>(), d_tot.as<uint32_t>());
    (void)hipMemcpyAsync(out, d_out.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st);
    (void)hipMemcpyAsync(out_wg, d_wg.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st);
    (void)hipMemcpyAsync(wg_total, d_tot.p, 4 * (size_t)wgs, hipMemcpyDeviceToHost, st);
    return test_finish(c);
  });
}

// table: n_recs edit records, the sentinel among them; the check pass of the Text calls (am355_textrec.h rec_premises) runs over the R
// records from `begin` on. *flags: the premise bits; *length: what the word held before the call, and after it.
static int test_premises(am355_ctx* c, const char* who, void (*launch)(const TextRecs&, uint32_t*, hipStream_t), const am355_ir_edit* table, uint32_t n_recs, uint32_t begin,
                         uint32_t R, uint32_t n_values, uint32_t* flags, uint32_t* length) {
  if (!c || !table || !flags || !length) return AM355_E_ARG;
  return guarded(c, [&]() -> int {
    if (!R || (uint64_t)begin + R + 1 > n_recs) return fail(c, AM355_E_ARG, "%s: the records (and the one behind them) leave the table", who);
    (void)hipSetDevice(c->device);
    hipStream_t st = c->stream;
    TestImage dt, dw;
    uint32_t words[2] = {0u, *length};
    if (!dt.up(table, sizeof(am355_ir_edit) * (size_t)n_recs, st) || !dw.up(words, 8, st)) return fail(c, AM355_E_NOMEM, "alloc");
    launch(TextRecs{(const am355_ir_edit*)dt.p, begin, R, n_values}, dw.words(), st);
    dw.down(words, st);
    int rc = test_finish(c);
    if (rc != AM355_OK) return rc;
    *flags = words[0];
    *length = words[1];
    return AM355_OK;
  });
}
extern "C" int am355_test_text_premises(am355_ctx* c, const am355_ir_edit* table, uint32_t n_recs, uint32_t begin, uint32_t R, uint32_t n_values, uint32_t* flags,
                                        uint32_t* length) {
  return test_premises(c, "am355_test_text_premises", launch_text_check, table, n_recs, begin, R, n_values, flags, length);
}
// the same over the check pass of the calls on a plain list (am355_list_locate.hip klist_check)
extern "C" int am355_test_list_premises(am355_ctx* c, const am355_ir_edit* table, uint32_t n_recs, uint32_t begin, uint32_t R, uint32_t n_values, uint32_t* flags,
                                        uint32_t* length) {
  return test_premises(c, "am355_test_list_premises", launch_list_check, table, n_recs, begin, R, n_values, flags, length);
}

extern "C" int am355_get_rows(am355_ctx* c, uint32_t* obj_actor, uint32_t* obj_ctr, uint32_t* key_actor, uint32_t* key_ctr, uint32_t* key_off,
                              uint32_t* key_len, uint32_t* action, uint32_t* val_tl, uint32_t* val_off, uint32_t* pred_num, uint32_t* id_ctr,
                              uint32_t* id_actor, uint8_t* insert, uint32_t* succ_cnt) {
  if (!c || !c->replayed) return AM355_E_STATE;
  if (c->shard_world > 1) return fail(c, AM355_E_UNSUPPORTED, "am355_get_rows on a sharded context (foreign rows are decoded as far as their object columns only)");
  (void)hipSetDevice(c->device);
  size_t N = c->n_ops;
  hipStream_t st = c->stream;
  auto pull = [&](void* dst, const void* src, size_t bytes) { if (dst && bytes) (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st); };
  pull(obj_actor, c->cols.obj_actor, 4 * N); pull(obj_ctr, c->cols.obj_ctr, 4 * N); pull(key_actor, c->cols.key_actor, 4 * N);
  pull(key_ctr, c->cols.key_ctr, 4 * N); pull(key_off, c->cols.key_off, 4 * N); pull(key_len, c->cols.key_len, 4 * N);
  pull(action, c->cols.action, 4 * N); pull(val_tl, c->cols.val_tl, 4 * N); pull(val_off, c->cols.val_off, 4 * N);
  pull(pred_num, c->cols.pred_num, 4 * N); pull(id_ctr, c->cols.id_ctr, 4 * N); pull(id_actor, c->cols.id_actor, 4 * N);
  pull(insert, c->cols.insert, N); pull(succ_cnt, c->mb.succ_cnt, 4 * N);
  HIPCHK(c, hipStreamSynchronize(st));
  return AM355_OK;
}

extern "C" int am355_load_changes(am355_ctx* c, const uint8_t* arena, const uint64_t* offsets, uint32_t n) { return guarded(c, [&]() { return load_changes_impl(c, arena, offsets, n); }); }
extern "C" int am355_load_document(am355_ctx* c, const uint8_t* doc, size_t len) { return guarded(c, [&]() { return load_document_impl(c, doc, len); }); }
extern "C" int am355_backend_load(am355_ctx* c, const uint8_t* doc, size_t len) { return guarded(c, [&]() { return backend_load_impl(c, doc, len); }); }
extern "C" int am355_replay(am355_ctx* c) { return guarded(c, [&]() { return replay_impl(c); }); }
extern "C" int am355_fetch_ir(am355_ctx* c, am355_patch_ir* out) { return guarded(c, [&]() { return fetch_ir_impl(c, out); }); }
extern "C" int am355_patch_json(am355_ctx* c, const char** json, size_t* len) { return guarded(c, [&]() { return patch_json_impl(c, json, len); }); }
extern "C" int am355_save(am355_ctx* c, uint32_t flags, const uint8_t** out_bytes, size_t* out_len) { return guarded(c, [&]() { return save_impl(c, flags, out_bytes, out_len); }); }
extern "C" int am355_doc_changes(am355_ctx* c, uint32_t flags, const uint8_t** arena, const uint64_t** offsets, uint32_t* n, const uint8_t** hashes) { return guarded(c, [&]() { return doc_changes_impl(c, flags, arena, offsets, n, hashes); }); }
extern "C" int am355_import_fragments(am355_ctx* c, const uint8_t* frags, const uint64_t* offsets, uint32_t world) { return guarded(c, [&]() { return import_fragments_impl(c, frags, offsets, world); }); }
extern "C" int am355_apply_changes(am355_ctx* c, const uint8_t* arena, const uint64_t* offsets, uint32_t n) { return guarded(c, [&]() { return apply_changes_impl(c, arena, offsets, n); }); }
extern "C" int am355_encode_change(am355_ctx* c, const am355_local_change* lc, const uint8_t** bytes, size_t* len, uint8_t hash[32]) { return guarded(c, [&]() { return encode_change_impl(c, lc, bytes, len, hash); }); }
extern "C" int am355_apply_local_change(am355_ctx* c, const am355_local_change* lc, const uint8_t** change, size_t* len) { return guarded(c, [&]() { return apply_local_change_impl(c, lc, change, len); }); }
extern "C" int am355_apply_patch_json(am355_ctx* c, const char** json, size_t* len) { return guarded(c, [&]() { return apply_patch_json_impl(c, json, len); }); }
extern "C" int am355_get_dep_graph(am355_ctx* c, const uint32_t** dep_first, const uint32_t** dep_index, uint32_t* n) { return guarded(c, [&]() { return get_dep_graph_impl(c, dep_first, dep_index, n); }); }
extern "C" int am355_sync_bloom_build(am355_ctx* c, const uint32_t* idx, uint32_t n, uint8_t* bits, size_t cap) {
  return guarded(c, [&]() { return sync_bloom_impl(c, idx, n, n, 10, 7, nullptr, 0, bits, cap, true); });
}
extern "C" int am355_sync_bloom_probe(am355_ctx* c, const uint32_t* idx, uint32_t n, uint32_t num_entries, uint32_t bits_per_entry, uint32_t num_probes, const uint8_t* bits,
                                      size_t n_bytes, uint8_t* contains) {
  return guarded(c, [&]() { return sync_bloom_impl(c, idx, n, num_entries, bits_per_entry, num_probes, bits, n_bytes, contains, n, false); });
}

