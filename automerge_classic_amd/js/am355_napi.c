/*
 * am355_napi.c -- thin N-API (v8, Node >= 12) binding of the C ABI in include/am355.h.
 *
 * The reference has no native addon; this is the binding a maintainer adds so that the unchanged JavaScript
 * frontend can call the MI355X engine through `Automerge.setDefaultBackend(require('mi355x-backend'))`
 * (reference plug-in point: src/automerge.js:147-149; harness: test/wasm.js:12-25).  One JS function per C entry
 * point, no logic of its own.
 *
 *   const am = require('./am355_napi.node')
 *   const ctx = am.create(0)                       // throws if no MI355X is usable (no CPU fallback)
 *   am.loadChanges(ctx, [Uint8Array, ...])         // stage + inflate + copy to HBM
 *   am.loadDocument(ctx, Uint8Array)               // stage one saved document (Backend.save bytes)
 *   am.backendLoad(ctx, Uint8Array)                // Backend.load in one call: loadDocument + replay, checksum beside the device stages
 *   am.replay(ctx)                                 // the hot path (blocking, like every Backend call)
 *   am.patchJSON(ctx) -> string                    // JSON.stringify(getPatch) text, built from the device IR
 *   am.fetchIR(ctx[, reuse]) -> {objects, map, edits, arena, ...}  // the record tables; materialize.js builds the patch object.
 *                                                  // reuse = true: into the context's own ArrayBuffers (valid until its next fetchIR)
 *   am.stats(ctx) -> {nOps, nChanges, msTotal, ...};  am.hashes(ctx) -> Uint8Array(32 * n);  am.destroy(ctx)
 */
#include <node_api.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/am355.h"

#define NAPI_CALL(env, call)                                                   \
  do {                                                                         \
    if ((call) != napi_ok) {                                                   \
      napi_throw_error((env), NULL, "N-API call failed: " #call);              \
      return NULL;                                                             \
    }                                                                          \
  } while (0)

/* the external wraps a small box so that an explicit destroy() and the finalizer cannot both release the context */
/* It also keeps what the binding reuses from call to call on a context: the gather buffer of loadChanges / applyChanges (a fresh
 * 13 MB malloc per call cost more in page faults than the copy itself) and, for fetchIR(ctx, true), the JS ArrayBuffers the record
 * tables are copied into. */
enum { IR_OBJECTS = 0, IR_MAP, IR_EDITS, IR_ARENA, IR_SLOTS };
typedef struct {
  am355_ctx *ctx;
  uint8_t *gather; size_t gather_cap;
  uint64_t *offsets; size_t offsets_cap;
  napi_ref ir_ref[IR_SLOTS]; size_t ir_cap[IR_SLOTS];
  uint64_t arena_epoch; size_t arena_copied;   /* what the reusable arena buffer mirrors: bytes [0, arena_copied) of the arena of that epoch */
} ctx_box;

static void finalize_ctx(napi_env env, void *data, void *hint) {
  (void)hint;
  ctx_box *box = (ctx_box *)data;
  if (!box) return;
  if (box->ctx) am355_destroy(box->ctx);
  for (int k = 0; k < IR_SLOTS; k++)
    if (box->ir_ref[k]) napi_delete_reference(env, box->ir_ref[k]);
  free(box->gather);
  free(box->offsets);
  free(box);
}

static ctx_box *get_box(napi_env env, napi_value v) {
  void *p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((ctx_box *)p)->ctx) {
    napi_throw_type_error(env, NULL, "expected a live am355 context");
    return NULL;
  }
  return (ctx_box *)p;
}

static am355_ctx *get_ctx(napi_env env, napi_value v) {
  void *p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((ctx_box *)p)->ctx) {
    napi_throw_type_error(env, NULL, "expected a live am355 context");
    return NULL;
  }
  return ((ctx_box *)p)->ctx;
}

static napi_value throw_engine(napi_env env, am355_ctx *ctx, int rc) {
  /* error object carries the code and the validity flags so the JS wrapper can decide to replay on the JS path */
  napi_value msg, err, code, flags;
  napi_create_string_utf8(env, am355_last_error(ctx), NAPI_AUTO_LENGTH, &msg);
  napi_create_error(env, NULL, msg, &err);
  napi_create_int32(env, rc, &code);
  napi_create_uint32(env, am355_flags(ctx), &flags);
  napi_set_named_property(env, err, "am355Code", code);
  napi_set_named_property(env, err, "am355Flags", flags);
  napi_throw(env, err);
  return NULL;
}

static napi_value js_create(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t device = 0;
  if (argc >= 1) napi_get_value_int32(env, argv[0], &device);
  am355_ctx *ctx = am355_create(device);
  if (!ctx) {
    napi_throw_error(env, NULL, "am355_create failed: no usable MI355X / HIP device (the engine has no CPU fallback)");
    return NULL;
  }
  ctx_box *box = (ctx_box *)calloc(1, sizeof(ctx_box));
  if (!box) { am355_destroy(ctx); napi_throw_error(env, NULL, "out of memory"); return NULL; }
  box->ctx = ctx;
  napi_value ext;
  NAPI_CALL(env, napi_create_external(env, box, finalize_ctx, NULL, &ext));
  return ext;
}

static napi_value js_destroy(napi_env env, napi_callback_info info) {
  /* releases the engine context now; the finalizer of the external then finds an empty box */
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *p = NULL;
  if (argc >= 1 && napi_get_value_external(env, argv[0], &p) == napi_ok && p && ((ctx_box *)p)->ctx) {
    am355_destroy(((ctx_box *)p)->ctx);
    ((ctx_box *)p)->ctx = NULL;
  }
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}

/* loadChanges(ctx, changes) = am355_load_changes; applyChanges(ctx, changes) = am355_apply_changes (Backend.applyChanges onto the
 * state the context holds: the incremental patch is then read with fetchApplyIR / applyPatchJSON) */
static napi_value stage_changes(napi_env env, napi_callback_info info, int apply) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ctx_box *box = get_box(env, argv[0]);
  if (!box) return NULL;
  am355_ctx *ctx = box->ctx;
  bool is_array = false;
  napi_is_array(env, argv[1], &is_array);
  if (!is_array) { napi_throw_type_error(env, NULL, "applyChanges takes an array of Uint8Arrays"); return NULL; }
  uint32_t n = 0;
  napi_get_array_length(env, argv[1], &n);
  if (box->offsets_cap < (size_t)n + 1) {
    size_t cap = ((size_t)n + 1) * 2;
    uint64_t *q = (uint64_t *)realloc(box->offsets, sizeof(uint64_t) * cap);
    if (!q) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    box->offsets = q; box->offsets_cap = cap;
  }
  uint64_t *offsets = box->offsets;
  /* ONE pass over the array: every change is copied behind the one in front as its typed-array info arrives (two N-API calls per
   * change; the first version made five and went over the array twice) */
  size_t total = 0;
  offsets[0] = 0;
  for (uint32_t i = 0; i < n; i++) {
    napi_value el;
    napi_typedarray_type t; size_t len; void *data; napi_value ab; size_t off;
    if (napi_get_element(env, argv[1], i, &el) != napi_ok || napi_get_typedarray_info(env, el, &t, &len, &data, &ab, &off) != napi_ok || t != napi_uint8_array) {
      napi_throw_type_error(env, NULL, "change is not a Uint8Array");
      return NULL;
    }
    if (total + len > box->gather_cap) {
      size_t cap = (total + len) * 2 + 4096;
      uint8_t *q = (uint8_t *)realloc(box->gather, cap);
      if (!q) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
      box->gather = q; box->gather_cap = cap;
    }
    if (len) memcpy(box->gather + total, data, len);
    total += len;
    offsets[i + 1] = total;
  }
  static const uint8_t none = 0;
  int rc = apply ? am355_apply_changes(ctx, total ? box->gather : &none, offsets, n) : am355_load_changes(ctx, total ? box->gather : &none, offsets, n);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}
static napi_value js_load_changes(napi_env env, napi_callback_info info) { return stage_changes(env, info, 0); }
static napi_value js_apply_changes(napi_env env, napi_callback_info info) { return stage_changes(env, info, 1); }

static napi_value js_load_document(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  bool is_ta = false;
  napi_is_typedarray(env, argv[1], &is_ta);
  if (!is_ta) { napi_throw_type_error(env, NULL, "document is not a Uint8Array"); return NULL; }
  napi_typedarray_type t; size_t len; void *data; napi_value ab; size_t off;
  napi_get_typedarray_info(env, argv[1], &t, &len, &data, &ab, &off);
  if (t != napi_uint8_array) { napi_throw_type_error(env, NULL, "document is not a Uint8Array"); return NULL; }
  int rc = am355_load_document(ctx, (const uint8_t *)data, len);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}

static napi_value js_backend_load(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  bool is_ta = false;
  napi_is_typedarray(env, argv[1], &is_ta);
  if (!is_ta) { napi_throw_type_error(env, NULL, "document is not a Uint8Array"); return NULL; }
  napi_typedarray_type t; size_t len; void *data; napi_value ab; size_t off;
  napi_get_typedarray_info(env, argv[1], &t, &len, &data, &ab, &off);
  if (t != napi_uint8_array) { napi_throw_type_error(env, NULL, "document is not a Uint8Array"); return NULL; }
  int rc = am355_backend_load(ctx, (const uint8_t *)data, len);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}

static napi_value js_replay(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int rc = am355_replay(ctx);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}

static napi_value js_patch_json(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  const char *json = NULL;
  size_t len = 0;
  int rc = am355_patch_json(ctx, &json, &len);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value s;
  NAPI_CALL(env, napi_create_string_utf8(env, json, len, &s));
  return s;
}

/* save(ctx, flags) -> Uint8Array: am355_save (Backend.save, new.js:2033-2055); the bytes are copied into a JS-owned buffer */
static napi_value js_save(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t flags = 0;
  if (argc > 1) napi_get_value_uint32(env, argv[1], &flags);
  const uint8_t *bytes = NULL;
  size_t len = 0;
  int rc = am355_save(ctx, flags, &bytes, &len);
  if (rc) return throw_engine(env, ctx, rc);
  void *data = NULL;
  napi_value ab, ta;
  NAPI_CALL(env, napi_create_arraybuffer(env, len, &data, &ab));
  if (len) memcpy(data, bytes, len);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta));
  return ta;
}

/* appliedOrder(ctx) -> Uint32Array: input indexes of the applied changes in application order (am355_get_applied) */
static napi_value js_applied_order(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t n = 0;
  int rc = am355_get_applied(ctx, NULL, &n);
  if (rc) return throw_engine(env, ctx, rc);
  void *data = NULL;
  napi_value ab, ta;
  NAPI_CALL(env, napi_create_arraybuffer(env, 4 * (size_t)n, &data, &ab));
  rc = am355_get_applied(ctx, (uint32_t *)data, &n);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n, ab, 0, &ta));
  return ta;
}

/* appliedInInputOrder(ctx) -> boolean: every staged change applied, in staged order, none queued (am355_applied_in_input_order) */
static napi_value js_applied_in_input_order(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int yes = 0;
  int rc = am355_applied_in_input_order(ctx, &yes);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_get_boolean(env, yes != 0, &out));
  return out;
}

/* forgetCallHistory(ctx, docChanges): am355_forget_call_history (the staged changes were replayed in one go, not by the calls that built the state) */
static napi_value js_forget_call_history(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t doc_changes = 0;  /* how many of the leading staged changes are the rebuilt history of a loaded document (0: none) */
  if (argc > 1) NAPI_CALL(env, napi_get_value_uint32(env, argv[1], &doc_changes));
  int rc = am355_forget_call_history(ctx, (int)doc_changes);
  if (rc) return throw_engine(env, ctx, rc);
  return NULL;
}

/* setResidentNewActors(ctx, on): am355_set_resident_new_actors (the first changes of a new actor are merged into the state the context
   holds instead of taking the full replay) */
static napi_value js_set_resident_new_actors(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  bool on = true;
  if (argc > 1) NAPI_CALL(env, napi_get_value_bool(env, argv[1], &on));
  int rc = am355_set_resident_new_actors(ctx, on ? 1 : 0);
  if (rc) return throw_engine(env, ctx, rc);
  return NULL;
}

/* setResidentMapMerge(ctx, on): am355_set_resident_map_merge (the plain map rows of a batch are merged into the stored map records of the
   state the context holds instead of every record being emitted and ordered again) */
static napi_value js_set_resident_map_merge(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  bool on = true;
  if (argc > 1) NAPI_CALL(env, napi_get_value_bool(env, argv[1], &on));
  int rc = am355_set_resident_map_merge(ctx, on ? 1 : 0);
  if (rc) return throw_engine(env, ctx, rc);
  return NULL;
}

/* residentMapMergeCalls(ctx) -> [merged in place, tried and declined]: am355_resident_map_merge_calls */
static napi_value js_resident_map_merge_calls(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint64_t w[2] = {0, 0};
  int rc = am355_resident_map_merge_calls(ctx, w);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_array_with_length(env, 2, &out));
  for (uint32_t k = 0; k < 2; k++) {
    NAPI_CALL(env, napi_create_double(env, (double)w[k], &v));
    NAPI_CALL(env, napi_set_element(env, out, k, v));
  }
  return out;
}

/* setResidentNewObjects(ctx, on): am355_set_resident_new_objects (a batch that makes objects is merged into the state the context holds in
   place instead of every list being ranked and every table rebuilt) */
static napi_value js_set_resident_new_objects(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  bool on = true;
  if (argc > 1) NAPI_CALL(env, napi_get_value_bool(env, argv[1], &on));
  int rc = am355_set_resident_new_objects(ctx, on ? 1 : 0);
  if (rc) return throw_engine(env, ctx, rc);
  return NULL;
}

/* residentNewObjectCalls(ctx) -> [served in place, tried and declined]: am355_resident_new_object_calls */
static napi_value js_resident_new_object_calls(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint64_t w[2] = {0, 0};
  int rc = am355_resident_new_object_calls(ctx, w);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_array_with_length(env, 2, &out));
  for (uint32_t k = 0; k < 2; k++) {
    NAPI_CALL(env, napi_create_double(env, (double)w[k], &v));
    NAPI_CALL(env, napi_set_element(env, out, k, v));
  }
  return out;
}

/* setResidentCounters(ctx, on): am355_set_resident_counters (the increments of map counters in a batch are written into the stored map
   records in place instead of every list being ranked and every table rebuilt) */
static napi_value js_set_resident_counters(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  bool on = true;
  if (argc > 1) NAPI_CALL(env, napi_get_value_bool(env, argv[1], &on));
  int rc = am355_set_resident_counters(ctx, on ? 1 : 0);
  if (rc) return throw_engine(env, ctx, rc);
  return NULL;
}

/* residentCounterCalls(ctx) -> [served in place, tried and declined]: am355_resident_counter_calls */
static napi_value js_resident_counter_calls(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint64_t w[2] = {0, 0};
  int rc = am355_resident_counter_calls(ctx, w);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_array_with_length(env, 2, &out));
  for (uint32_t k = 0; k < 2; k++) {
    NAPI_CALL(env, napi_create_double(env, (double)w[k], &v));
    NAPI_CALL(env, napi_set_element(env, out, k, v));
  }
  return out;
}

/* hashGraphKnown(ctx, set) -> boolean: am355_hash_graph_known (set: 1 / 0 / -1 = only ask) */
static napi_value js_hash_graph_known(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int32_t set = -1;
  if (argc > 1) NAPI_CALL(env, napi_get_value_int32(env, argv[1], &set));
  int known = 1;
  int rc = am355_hash_graph_known(ctx, (int)set, &known);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value out;
  NAPI_CALL(env, napi_get_boolean(env, known != 0, &out));
  return out;
}

/* pendingOrder(ctx) -> Uint32Array: am355_get_pending (the changes still queued, as indexes into the engine's list of changes) */
static napi_value js_pending_order(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t n = 0;
  int rc = am355_get_pending(ctx, NULL, &n);
  if (rc) return throw_engine(env, ctx, rc);
  void *data = NULL;
  napi_value ab, ta;
  NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)n * 4, &data, &ab));
  if (n) am355_get_pending(ctx, (uint32_t *)data, &n);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n, ab, 0, &ta));
  return ta;
}

static napi_value copy_to_arraybuffer(napi_env env, const void *src, size_t len);

static int get_u32_array(napi_env env, napi_value v, uint32_t **data, size_t *n) {
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (!is_ta) return 0;
  napi_typedarray_type t; size_t len; void *d; napi_value ab; size_t off;
  napi_get_typedarray_info(env, v, &t, &len, &d, &ab, &off);
  if (t != napi_uint32_array) return 0;
  *data = (uint32_t *)d;
  *n = len;
  return 1;
}

/* depGraph(ctx) -> { depFirst: Uint32Array[n + 1], depIndex: Uint32Array }: am355_get_dep_graph (copies) */
static napi_value js_dep_graph(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  const uint32_t *first = NULL, *index = NULL;
  uint32_t n = 0;
  int rc = am355_get_dep_graph(ctx, &first, &index, &n);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value o, ab, ta;
  NAPI_CALL(env, napi_create_object(env, &o));
  ab = copy_to_arraybuffer(env, first, 4 * ((size_t)n + 1));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, (size_t)n + 1, ab, 0, &ta));
  napi_set_named_property(env, o, "depFirst", ta);
  ab = copy_to_arraybuffer(env, index, 4 * (size_t)first[n]);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, first[n], ab, 0, &ta));
  napi_set_named_property(env, o, "depIndex", ta);
  return o;
}

/* hashes packed 32 bytes each in a Uint8Array (a view is fine): the pointer and how many; 0 when the argument is no such array */
static int get_hash_array(napi_env env, napi_value v, const uint8_t **data, uint32_t *n) {
  bool is_ta = false;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return 0;
  napi_typedarray_type t; size_t len; void *d; napi_value ab; size_t off;
  if (napi_get_typedarray_info(env, v, &t, &len, &d, &ab, &off) != napi_ok || t != napi_uint8_array || len % 32 != 0 || len / 32 > 0xffffffffu) return 0;
  *data = (const uint8_t *)d;
  *n = (uint32_t)(len / 32);
  return 1;
}

/* findChanges(ctx, Uint8Array hashes) -> Uint32Array: am355_find_changes (0xffffffff: no applied change has that hash) */
static napi_value js_find_changes(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  const uint8_t *hashes = NULL;
  uint32_t n = 0;
  if (argc < 2 || !get_hash_array(env, argv[1], &hashes, &n)) { napi_throw_type_error(env, NULL, "findChanges takes a Uint8Array of 32-byte hashes"); return NULL; }
  void *data = NULL;
  napi_value ab, ta;
  NAPI_CALL(env, napi_create_arraybuffer(env, 4 * (size_t)(n ? n : 1), &data, &ab));
  int rc = am355_find_changes(ctx, hashes, n, (uint32_t *)data);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n, ab, 0, &ta));
  return ta;
}

/* changesSince(ctx, Uint8Array have) / changesAdded(ctx, Uint8Array other) -> Uint32Array of indexes into the context's list of changes:
   am355_changes_since / am355_changes_added (copies) */
static napi_value index_query(napi_env env, napi_callback_info info, int (*fn)(am355_ctx *, const uint8_t *, uint32_t, const uint32_t **, uint32_t *), const char *usage) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  const uint8_t *hashes = NULL;
  uint32_t n = 0, n_out = 0;
  if (argc < 2 || !get_hash_array(env, argv[1], &hashes, &n)) { napi_throw_type_error(env, NULL, usage); return NULL; }
  const uint32_t *idx = NULL;
  int rc = fn(ctx, hashes, n, &idx, &n_out);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value ab = copy_to_arraybuffer(env, idx, 4 * (size_t)n_out), ta;
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n_out, ab, 0, &ta));
  return ta;
}
static napi_value js_changes_since(napi_env env, napi_callback_info info) { return index_query(env, info, am355_changes_since, "changesSince takes a Uint8Array of 32-byte hashes"); }
static napi_value js_changes_added(napi_env env, napi_callback_info info) { return index_query(env, info, am355_changes_added, "changesAdded takes a Uint8Array of 32-byte hashes"); }

/* missingDeps(ctx, Uint8Array heads) -> Uint8Array of 32-byte hashes, sorted: am355_missing_deps (copies) */
static napi_value js_missing_deps(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  const uint8_t *heads = NULL, *out = NULL;
  uint32_t n = 0, n_out = 0;
  if (argc < 2 || !get_hash_array(env, argv[1], &heads, &n)) { napi_throw_type_error(env, NULL, "missingDeps takes a Uint8Array of 32-byte hashes"); return NULL; }
  int rc = am355_missing_deps(ctx, heads, n, &out, &n_out);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value ab = copy_to_arraybuffer(env, out, 32 * (size_t)n_out), ta;
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, 32 * (size_t)n_out, ab, 0, &ta));
  return ta;
}

/* setGraphProbeMin(ctx, n): am355_set_graph_probe_min (0xffffffff: the membership tests of the queries above never go to the device) */
static napi_value js_set_graph_probe_min(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t n = 0xffffffffu;
  if (argc > 1) NAPI_CALL(env, napi_get_value_uint32(env, argv[1], &n));
  int rc = am355_set_graph_probe_min(ctx, n);
  if (rc) return throw_engine(env, ctx, rc);
  return NULL;
}

/* graphQueryCalls(ctx) -> [membership tests on the device, by the host index]: am355_graph_query_calls */
static napi_value js_graph_query_calls(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint64_t w[2] = {0, 0};
  int rc = am355_graph_query_calls(ctx, w);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_array_with_length(env, 2, &out));
  for (uint32_t k = 0; k < 2; k++) {
    NAPI_CALL(env, napi_create_double(env, (double)w[k], &v));
    NAPI_CALL(env, napi_set_element(env, out, k, v));
  }
  return out;
}

/* objectText(ctx, ctr, Uint8Array actor) -> {text, length, strings}: am355_object_text (the string of a Text object read on the device;
 * text: the pinned bytes as a JS string, length: the object's list length, strings: its elements that are strings) */
static napi_value js_object_text(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], out, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double ctr = -1;
  bool is_ta = false;
  if (argc < 3 || napi_get_value_double(env, argv[1], &ctr) != napi_ok || napi_is_typedarray(env, argv[2], &is_ta) != napi_ok || !is_ta || ctr < 0 || ctr > 4294967295.0) {
    napi_throw_type_error(env, NULL, "objectText takes a counter and the actor's bytes");
    return NULL;
  }
  napi_typedarray_type t;
  size_t n = 0;
  void *actor = NULL;
  NAPI_CALL(env, napi_get_typedarray_info(env, argv[2], &t, &n, &actor, NULL, NULL));
  if (t != napi_uint8_array) { napi_throw_type_error(env, NULL, "objectText takes a counter and the actor's bytes"); return NULL; }
  const uint8_t *utf8 = NULL;
  size_t len = 0;
  am355_text_info ti;
  int rc = am355_object_text(ctx, (uint64_t)ctr, (const uint8_t *)actor, n, &utf8, &len, &ti);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_object(env, &out));
  NAPI_CALL(env, napi_create_string_utf8(env, len ? (const char *)utf8 : "", len, &v));
  NAPI_CALL(env, napi_set_named_property(env, out, "text", v));
  NAPI_CALL(env, napi_create_uint32(env, ti.n_elements, &v));
  NAPI_CALL(env, napi_set_named_property(env, out, "length", v));
  NAPI_CALL(env, napi_create_uint32(env, ti.n_strings, &v));
  NAPI_CALL(env, napi_set_named_property(env, out, "strings", v));
  return out;
}

/* bloomBuild(ctx, Uint32Array idx) -> Uint8Array: am355_sync_bloom_build (the `bits` of the filter over those changes' hashes) */
static napi_value js_bloom_build(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t *idx = NULL;
  size_t n = 0;
  if (!get_u32_array(env, argv[1], &idx, &n)) { napi_throw_type_error(env, NULL, "bloomBuild takes a Uint32Array of change indexes"); return NULL; }
  size_t bytes = (n * 10 + 7) / 8;
  void *data = NULL;
  napi_value ab, ta;
  NAPI_CALL(env, napi_create_arraybuffer(env, bytes, &data, &ab));
  int rc = am355_sync_bloom_build(ctx, idx, (uint32_t)n, (uint8_t *)data, bytes);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, bytes, ab, 0, &ta));
  return ta;
}

/* bloomProbe(ctx, Uint32Array idx, numEntries, numBitsPerEntry, numProbes, Uint8Array bits) -> Uint8Array flags: am355_sync_bloom_probe */
static napi_value js_bloom_probe(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t *idx = NULL;
  size_t n = 0;
  if (!get_u32_array(env, argv[1], &idx, &n)) { napi_throw_type_error(env, NULL, "bloomProbe takes a Uint32Array of change indexes"); return NULL; }
  uint32_t ne = 0, nb = 0, np = 0;
  napi_get_value_uint32(env, argv[2], &ne); napi_get_value_uint32(env, argv[3], &nb); napi_get_value_uint32(env, argv[4], &np);
  bool is_ta = false;
  napi_is_typedarray(env, argv[5], &is_ta);
  if (!is_ta) { napi_throw_type_error(env, NULL, "filter bits must be a Uint8Array"); return NULL; }
  napi_typedarray_type t; size_t blen; void *bdata; napi_value bab; size_t boff;
  napi_get_typedarray_info(env, argv[5], &t, &blen, &bdata, &bab, &boff);
  if (t != napi_uint8_array) { napi_throw_type_error(env, NULL, "filter bits must be a Uint8Array"); return NULL; }
  void *data = NULL;
  napi_value ab, ta;
  NAPI_CALL(env, napi_create_arraybuffer(env, n ? n : 1, &data, &ab));
  int rc = am355_sync_bloom_probe(ctx, idx, (uint32_t)n, ne, nb, np, (const uint8_t *)bdata, blen, (uint8_t *)data);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta));
  return ta;
}

static napi_value js_reset(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int rc = am355_reset(ctx);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}

/* hashes(ctx[, first]) -> Uint8Array: the hashes of changes [first, n_changes), 32 bytes each (first = 0: all of them) */
static napi_value js_hashes(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t first = 0;
  if (argc > 1) (void)napi_get_value_uint32(env, argv[1], &first);
  am355_stats st;
  am355_get_stats(ctx, &st);
  if (first > st.n_changes) { napi_throw_range_error(env, NULL, "hashes: first beyond the staged changes"); return NULL; }
  void *data = NULL;
  napi_value ab, ta;
  size_t bytes = 32 * (size_t)(st.n_changes - first);
  NAPI_CALL(env, napi_create_arraybuffer(env, bytes, &data, &ab));
  int rc = am355_get_hashes_range(ctx, first, st.n_changes - first, (uint8_t *)data);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, bytes, ab, 0, &ta));
  return ta;
}

static void set_num(napi_env env, napi_value obj, const char *name, double v) {
  napi_value n;
  napi_create_double(env, v, &n);
  napi_set_named_property(env, obj, name, n);
}


/* copy `len` bytes into a JS-owned ArrayBuffer (the engine's pinned buffers are reused by the next call on the context) */
static napi_value copy_to_arraybuffer(napi_env env, const void *src, size_t len) {
  void *data = NULL;
  napi_value ab;
  if (napi_create_arraybuffer(env, len, &data, &ab) != napi_ok) return NULL;
  if (len && src) memcpy(data, src, len);
  return ab;
}

/* fetchIR(ctx) -> {objects, map, edits, arena: ArrayBuffer, nObjects, nMap, nEdits, nValues, maxOp, pending,
 *                  actorOff: ArrayBuffer(u32), actorBytes: ArrayBuffer, clockActor: ArrayBuffer(u32), clockSeq: ArrayBuffer(f64), heads: ArrayBuffer}
 * am355_fetch_ir: the record tables of include/am355.h as the device wrote them; materialize.js builds the patch object. */
/* the table in a JS ArrayBuffer: a fresh one, or -- fetchIR(ctx, true) -- the context's own buffer for that table, grown when needed
 * (its content then changes with the next fetchIR on the context: for callers that materialise the patch at once, as index.js does) */
static napi_value ir_table(napi_env env, ctx_box *box, int slot, bool reuse, const void *src, size_t len) {
  if (!reuse) return copy_to_arraybuffer(env, src, len);
  napi_value ab = NULL;
  void *data = NULL;
  size_t have = 0;
  if (box->ir_ref[slot] && box->ir_cap[slot] >= len && napi_get_reference_value(env, box->ir_ref[slot], &ab) == napi_ok && ab &&
      napi_get_arraybuffer_info(env, ab, &data, &have) == napi_ok && have >= len) {
    if (len && src) memcpy(data, src, len);
    return ab;
  }
  if (box->ir_ref[slot]) { napi_delete_reference(env, box->ir_ref[slot]); box->ir_ref[slot] = NULL; box->ir_cap[slot] = 0; }
  size_t cap = (len + len / 4 + 4096 + 7) & ~(size_t)7;   /* (a multiple of 8: the JS side lays Uint32Array / Float64Array views over the whole buffer) */
  if (napi_create_arraybuffer(env, cap, &data, &ab) != napi_ok) return NULL;
  if (len && src) memcpy(data, src, len);
  if (napi_create_reference(env, ab, 1, &box->ir_ref[slot]) == napi_ok) box->ir_cap[slot] = cap;
  return ab;
}

/* The raw arena in the context's reusable buffer. Backend.applyChanges call after call appends a batch to the arena and keeps what is
 * there (am355_arena_epoch unchanged): only the new tail is copied -- the whole arena of a 1 M-op document is 13 MB, 0.3 ms of memcpy
 * per call for a batch of 3 KB. */
static napi_value arena_table(napi_env env, ctx_box *box, const void *src, size_t len) {
  uint64_t epoch = 0;
  napi_value ab = NULL;
  void *data = NULL;
  size_t have = 0;
  if (am355_arena_epoch(box->ctx, &epoch) == AM355_OK && epoch == box->arena_epoch && box->ir_ref[IR_ARENA] && box->ir_cap[IR_ARENA] >= len &&
      box->arena_copied <= len && napi_get_reference_value(env, box->ir_ref[IR_ARENA], &ab) == napi_ok && ab &&
      napi_get_arraybuffer_info(env, ab, &data, &have) == napi_ok && have >= len) {
    if (len > box->arena_copied && src) memcpy((uint8_t *)data + box->arena_copied, (const uint8_t *)src + box->arena_copied, len - box->arena_copied);
    box->arena_copied = len;
    return ab;
  }
  ab = ir_table(env, box, IR_ARENA, true, src, len);   /* (a new buffer comes with a quarter of room to grow into) */
  box->arena_epoch = epoch;
  box->arena_copied = ab ? len : 0;
  return ab;
}

static napi_value fetch_ir_common(napi_env env, napi_callback_info info, int apply) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ctx_box *box = get_box(env, argv[0]);
  if (!box) return NULL;
  am355_ctx *ctx = box->ctx;
  bool reuse = false;
  if (argc > 1) (void)napi_get_value_bool(env, argv[1], &reuse);
  am355_patch_ir ir;
  int rc = apply ? am355_fetch_apply_ir(ctx, &ir) : am355_fetch_ir(ctx, &ir);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
#define PUT_TAB(name, slot, ptr, bytes)                                                 \
  do {                                                                                  \
    napi_value ab_ = ir_table(env, box, (slot), reuse, (ptr), (bytes));                 \
    if (!ab_) { napi_throw_error(env, NULL, "out of memory (patch IR)"); return NULL; } \
    napi_set_named_property(env, o, name, ab_);                                         \
  } while (0)
#define PUT_AB(name, ptr, bytes)                                                        \
  do {                                                                                  \
    napi_value ab_ = copy_to_arraybuffer(env, (ptr), (bytes));                          \
    if (!ab_) { napi_throw_error(env, NULL, "out of memory (patch IR)"); return NULL; } \
    napi_set_named_property(env, o, name, ab_);                                         \
  } while (0)
  PUT_TAB("objects", IR_OBJECTS, ir.objects, (size_t)ir.n_objects * sizeof(am355_ir_object));
  PUT_TAB("map", IR_MAP, ir.map, (size_t)ir.n_map * sizeof(am355_ir_map));
  PUT_TAB("edits", IR_EDITS, ir.edits, ((size_t)ir.n_edits + 1) * sizeof(am355_ir_edit));
  if (reuse) {
    napi_value ab_ = arena_table(env, box, ir.arena, (size_t)ir.arena_len);
    if (!ab_) { napi_throw_error(env, NULL, "out of memory (patch IR)"); return NULL; }
    napi_set_named_property(env, o, "arena", ab_);
  } else PUT_TAB("arena", IR_ARENA, ir.arena, (size_t)ir.arena_len);
  PUT_AB("actorOff", ir.actor_off, ((size_t)ir.n_actors + 1) * sizeof(uint32_t));
  PUT_AB("actorBytes", ir.actor_bytes, ir.n_actors ? (size_t)ir.actor_off[ir.n_actors] : 0);
  PUT_AB("clockActor", ir.clock_actor, (size_t)ir.n_clock * sizeof(uint32_t));
  PUT_AB("heads", ir.heads, (size_t)ir.n_heads * 32);
  {
    void *data = NULL;
    napi_value ab;
    NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)ir.n_clock * sizeof(double), &data, &ab));
    for (uint32_t i = 0; i < ir.n_clock; i++) ((double *)data)[i] = (double)ir.clock_seq[i];
    napi_set_named_property(env, o, "clockSeq", ab);
  }
#undef PUT_AB
#undef PUT_TAB
  set_num(env, o, "nObjects", ir.n_objects); set_num(env, o, "nMap", ir.n_map); set_num(env, o, "nEdits", ir.n_edits);
  set_num(env, o, "nValues", ir.n_values); set_num(env, o, "nActors", ir.n_actors); set_num(env, o, "maxOp", (double)ir.max_op);
  set_num(env, o, "pending", ir.pending);
  am355_local_envelope local;
  if (apply && am355_apply_local_envelope(ctx, &local) == AM355_OK && local.is_local) {   /* the patch of applyLocalChange: actor and seq behind diffs; heads came without the change's own hash */
    set_num(env, o, "isLocal", 1); set_num(env, o, "localActor", local.actor); set_num(env, o, "localSeq", (double)local.seq);
  }
  return o;
}
static napi_value js_fetch_ir(napi_env env, napi_callback_info info) { return fetch_ir_common(env, info, 0); }
/* fetchApplyIR(ctx): the patch of the last applyChanges as record tables (am355_fetch_apply_ir) */
static napi_value js_fetch_apply_ir(napi_env env, napi_callback_info info) { return fetch_ir_common(env, info, 1); }

/* docChanges(ctx, flags) -> { changes: Uint8Array[], hashes: Uint8Array }: am355_doc_changes -- the history of a loaded document
 * (Backend.getAllChanges(Backend.load(bytes)), new.js:1887-1927). The changes are views into ONE JS-owned ArrayBuffer (the
 * reference's change buffers are views too: encoding.js Encoder.buffer), hashes holds 32 bytes per change. */
static napi_value js_doc_changes(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t flags = 1;
  if (argc > 1) napi_get_value_uint32(env, argv[1], &flags);
  const uint8_t *arena = NULL, *hashes = NULL;
  const uint64_t *offsets = NULL;
  uint32_t n = 0;
  int rc = am355_doc_changes(ctx, flags, &arena, &offsets, &n, &hashes);
  if (rc) return throw_engine(env, ctx, rc);
  size_t total = (size_t)offsets[n];
  void *data = NULL;
  napi_value ab, list, out, hab, hta;
  NAPI_CALL(env, napi_create_arraybuffer(env, total, &data, &ab));
  if (total) memcpy(data, arena, total);
  NAPI_CALL(env, napi_create_array_with_length(env, n, &list));
  for (uint32_t i = 0; i < n; i++) {
    napi_value ta;
    NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, (size_t)(offsets[i + 1] - offsets[i]), ab, (size_t)offsets[i], &ta));
    NAPI_CALL(env, napi_set_element(env, list, i, ta));
  }
  hab = copy_to_arraybuffer(env, hashes, 32 * (size_t)n);
  if (!hab) return NULL;
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, 32 * (size_t)n, hab, 0, &hta));
  NAPI_CALL(env, napi_create_object(env, &out));
  NAPI_CALL(env, napi_set_named_property(env, out, "changes", list));
  NAPI_CALL(env, napi_set_named_property(env, out, "hashes", hta));
  return out;
}

static napi_value js_stats(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  am355_stats st;
  am355_get_stats(ctx, &st);
  napi_value o;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_num(env, o, "nChanges", st.n_changes); set_num(env, o, "nApplied", st.n_applied); set_num(env, o, "nPending", st.n_pending);
  set_num(env, o, "nActors", st.n_actors); set_num(env, o, "nObjects", st.n_objects); set_num(env, o, "nOps", (double)st.n_ops);
  set_num(env, o, "maxOp", (double)st.max_op); set_num(env, o, "rawBytes", (double)st.raw_bytes); set_num(env, o, "nEdits", (double)st.n_edits);
  set_num(env, o, "msTotal", st.ms_total); set_num(env, o, "msParse", st.ms_parse); set_num(env, o, "msHostSchedule", st.ms_host_schedule);
  set_num(env, o, "msDecode", st.ms_decode); set_num(env, o, "msMerge", st.ms_merge); set_num(env, o, "msOrder", st.ms_order);
  set_num(env, o, "msHashStream", st.ms_hash_stream); set_num(env, o, "fastPath", st.fast_path);
  return o;
}

/* ---- objectId sharding with the collective inside the library (am355_shard_init / am355_sharded_replay: RCCL over xGMI) ----
 * shardUniqueId() -> Uint8Array(128)      rank 0's worker makes it; js/sharded.js hands it to the other workers (process.send)
 * shardInit(ctx, id, rank, world)         ncclCommInitRank on the context's GPU
 * shardedReplay(ctx, stitchOnAllRanks)    replay + ncclAllGather of the fragments + stitch; then patchJSON / fetchIR as usual
 * shardFragmentBytes(ctx, world) -> [..]  bytes each rank contributed;  shardFinalize(ctx)                                         */
static napi_value js_shard_unique_id(napi_env env, napi_callback_info info) {
  (void)info;
  void *data = NULL;
  napi_value ab, ta;
  NAPI_CALL(env, napi_create_arraybuffer(env, AM355_SHARD_ID_BYTES, &data, &ab));
  if (am355_shard_unique_id((uint8_t *)data) != AM355_OK) {
    napi_throw_error(env, NULL, "RCCL is not available (librccl.so.1, or AM355_RCCL_LIB)");
    return NULL;
  }
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, AM355_SHARD_ID_BYTES, ab, 0, &ta));
  return ta;
}

static napi_value js_shard_init(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  napi_typedarray_type ty;
  size_t len = 0, off = 0;
  void *data = NULL;
  napi_value ab;
  uint32_t rank = 0, world = 0;
  if (argc < 4 || napi_get_typedarray_info(env, argv[1], &ty, &len, &data, &ab, &off) != napi_ok || ty != napi_uint8_array || len != AM355_SHARD_ID_BYTES ||
      napi_get_value_uint32(env, argv[2], &rank) != napi_ok || napi_get_value_uint32(env, argv[3], &world) != napi_ok) {
    napi_throw_type_error(env, NULL, "shardInit(ctx, Uint8Array(128), rank, world)");
    return NULL;
  }
  int rc = am355_shard_init(ctx, (const uint8_t *)data, rank, world);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}

static napi_value js_sharded_replay(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  bool all = false;
  if (argc > 1) (void)napi_get_value_bool(env, argv[1], &all);
  int rc = am355_sharded_replay(ctx, all ? 1 : 0);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}

static napi_value js_shard_fragment_bytes(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t world = 0;
  if (argc < 2 || napi_get_value_uint32(env, argv[1], &world) != napi_ok || world == 0 || world > 4096) {
    napi_throw_type_error(env, NULL, "shardFragmentBytes(ctx, world)");
    return NULL;
  }
  uint64_t *bytes = (uint64_t *)calloc(world, sizeof(uint64_t));
  if (!bytes) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  int rc = am355_shard_fragment_bytes(ctx, bytes, world);
  if (rc) { free(bytes); return throw_engine(env, ctx, rc); }
  napi_value arr;
  napi_create_array_with_length(env, world, &arr);
  for (uint32_t r = 0; r < world; r++) {
    napi_value n;
    napi_create_double(env, (double)bytes[r], &n);
    napi_set_element(env, arr, r, n);
  }
  free(bytes);
  return arr;
}

static napi_value js_shard_finalize(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int rc = am355_shard_finalize(ctx);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value u;
  napi_get_undefined(env, &u);
  return u;
}

/* A change request as js/local_change.js flattens it: { seq, startOp, time, notFlat, message, deps, actorBytes, strings: Uint8Array,
 * actorOff, actorRank, ops (13 words per op), values (6 words per value: tag, off, len, 0, payload low, payload high), preds (2 words
 * per pred): Uint32Array } -> am355_local_change. No logic of its own: the arrays are handed over as they are. */
static bool flat_array(napi_env env, napi_value o, const char *name, size_t elem, const void **data, size_t *count) {
  napi_value v;
  napi_typedarray_type type;
  size_t length = 0;
  void *p = NULL;
  *data = NULL; *count = 0;
  if (napi_get_named_property(env, o, name, &v) != napi_ok || napi_get_typedarray_info(env, v, &type, &length, &p, NULL, NULL) != napi_ok) return false;
  if ((elem == 1 && type != napi_uint8_array) || (elem == 4 && type != napi_uint32_array)) return false;
  *data = p; *count = length;
  return true;
}
static bool flat_number(napi_env env, napi_value o, const char *name, double *out) {
  napi_value v;
  return napi_get_named_property(env, o, name, &v) == napi_ok && napi_get_value_double(env, v, out) == napi_ok;
}
static bool flat_request(napi_env env, napi_value o, am355_local_change *lc) {
  double seq = 0, start_op = 0, time = 0, not_flat = 0;
  const void *p;
  size_t n, n_off, n_rank;
  memset(lc, 0, sizeof *lc);
  if (!flat_number(env, o, "seq", &seq) || !flat_number(env, o, "startOp", &start_op) || !flat_number(env, o, "time", &time) || !flat_number(env, o, "notFlat", &not_flat)) return false;
  lc->not_flat = not_flat != 0 || seq < 0 || start_op < 0 || seq > 9007199254740991.0 || start_op > 9007199254740991.0 || time > 9007199254740991.0 || time < -9007199254740991.0;
  if (lc->not_flat) return true;
  lc->seq = (uint64_t)seq; lc->start_op = (uint64_t)start_op; lc->time = (int64_t)time;
  if (!flat_array(env, o, "message", 1, &p, &n)) return false;
  lc->message = (const uint8_t *)p; lc->message_len = (uint32_t)n;
  if (!flat_array(env, o, "deps", 1, &p, &n) || n % 32) return false;
  lc->deps = (const uint8_t *)p; lc->n_deps = (uint32_t)(n / 32);
  if (!flat_array(env, o, "actorOff", 4, &p, &n_off) || n_off < 2) return false;
  lc->actor_off = (const uint32_t *)p; lc->n_actors = (uint32_t)(n_off - 1);
  if (!flat_array(env, o, "actorRank", 4, &p, &n_rank) || n_rank != n_off - 1) return false;
  lc->actor_rank = (const uint32_t *)p;
  if (!flat_array(env, o, "actorBytes", 1, &p, &n) || n < lc->actor_off[lc->n_actors]) return false;
  lc->actor_bytes = (const uint8_t *)p;
  if (!flat_array(env, o, "strings", 1, &p, &n)) return false;
  lc->strings = (const uint8_t *)p; lc->strings_len = (uint32_t)n;
  if (!flat_array(env, o, "ops", 4, &p, &n) || n % (sizeof(am355_local_op) / 4)) return false;
  lc->ops = (const am355_local_op *)p; lc->n_ops = (uint32_t)(n / (sizeof(am355_local_op) / 4));
  if (!flat_array(env, o, "values", 4, &p, &n) || n % (sizeof(am355_local_value) / 4) || ((uintptr_t)p & 7)) return false;
  lc->values = (const am355_local_value *)p; lc->n_values = (uint32_t)(n / (sizeof(am355_local_value) / 4));
  if (!flat_array(env, o, "preds", 4, &p, &n) || n % 2) return false;
  lc->preds = (const am355_local_pred *)p; lc->n_preds = (uint32_t)(n / 2);
  return true;
}
/* encodeChange(ctx, flat) -> { change: Uint8Array, hash: Uint8Array(32) } = am355_encode_change;
 * applyLocalChange(ctx, flat) -> Uint8Array (the binary change) = am355_apply_local_change: the patch is then read with fetchApplyIR */
static napi_value local_change_common(napi_env env, napi_callback_info info, int apply) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  am355_local_change lc;
  if (argc < 2 || !flat_request(env, argv[1], &lc)) { napi_throw_type_error(env, NULL, "expected a flattened change request (js/local_change.js)"); return NULL; }
  const uint8_t *bytes = NULL;
  size_t len = 0;
  uint8_t hash[32];
  int rc = apply ? am355_apply_local_change(ctx, &lc, &bytes, &len) : am355_encode_change(ctx, &lc, &bytes, &len, hash);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value ab = copy_to_arraybuffer(env, bytes, len), change;
  if (!ab) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &change));
  if (apply) return change;
  napi_value o, hab = copy_to_arraybuffer(env, hash, 32), h;
  if (!hab) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, 32, hab, 0, &h));
  NAPI_CALL(env, napi_create_object(env, &o));
  napi_set_named_property(env, o, "change", change);
  napi_set_named_property(env, o, "hash", h);
  return o;
}
static napi_value js_encode_change(napi_env env, napi_callback_info info) { return local_change_common(env, info, 0); }
static napi_value js_apply_local_change(napi_env env, napi_callback_info info) { return local_change_common(env, info, 1); }
/* localChangeCalls(ctx) -> [served, refused] = am355_local_change_calls */
static napi_value js_local_change_calls(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint64_t out[2] = {0, 0};
  int rc = am355_local_change_calls(ctx, out);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value arr, v;
  NAPI_CALL(env, napi_create_array_with_length(env, 2, &arr));
  for (uint32_t k = 0; k < 2; k++) { napi_create_double(env, (double)out[k], &v); napi_set_element(env, arr, k, v); }
  return arr;
}

/* setLocalSmall(ctx, on): am355_set_local_small (a change request inside the limits of the path -- a keystroke, a pasted line -- is built
   by one workgroup in one launch instead of by the bulk encoders) */
static napi_value js_set_local_small(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  bool on = true;
  if (argc > 1) NAPI_CALL(env, napi_get_value_bool(env, argv[1], &on));
  int rc = am355_set_local_small(ctx, on ? 1 : 0);
  if (rc) return throw_engine(env, ctx, rc);
  return NULL;
}

/* localSmallCalls(ctx) -> [built by the one workgroup, switch on but outside the limits: bulk path] = am355_local_small_calls */
static napi_value js_local_small_calls(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint64_t out[2] = {0, 0};
  int rc = am355_local_small_calls(ctx, out);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value arr, v;
  NAPI_CALL(env, napi_create_array_with_length(env, 2, &arr));
  for (uint32_t k = 0; k < 2; k++) { napi_create_double(env, (double)out[k], &v); napi_set_element(env, arr, k, v); }
  return arr;
}

/* a Uint8Array argument: its bytes */
static bool get_u8_array(napi_env env, napi_value v, const uint8_t **p, size_t *n) {
  bool is_ta = false;
  napi_typedarray_type t;
  void *data = NULL;
  if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) return false;
  if (napi_get_typedarray_info(env, v, &t, n, &data, NULL, NULL) != napi_ok || t != napi_uint8_array) return false;
  *p = (const uint8_t *)data;
  return true;
}
/* "<ctr>@<actor in hex>" of an id whose actor is a rank of the engine's table (am355_actor_of_rank) */
static bool id_string(napi_env env, am355_ctx *ctx, uint32_t ctr, uint32_t rank, napi_value *out) {
  const uint8_t *a = NULL;
  size_t n = 0;
  char buf[16 + 2 * 256];
  if (am355_actor_of_rank(ctx, rank, &a, &n) != AM355_OK || n > 256) return false;
  int at = snprintf(buf, sizeof buf, "%u@", ctr);
  for (size_t k = 0; k < n; k++) at += snprintf(buf + at, 3, "%02x", a[k]);
  return napi_create_string_utf8(env, buf, (size_t)at, out) == napi_ok;
}
/* textLocate(ctx, ctr, Uint8Array actor, first, n) -> { length, runs: [{ elemId, pred, count, counter }] } = am355_text_locate: the
 * elements [first, first + n) of a Text as runs of consecutive (elemId, pred) pairs, ids as strings */
static napi_value js_text_locate(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5], out, runs_js, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double ctr = -1, first = -1, n = -1;
  const uint8_t *actor = NULL;
  size_t actor_len = 0;
  if (argc < 5 || napi_get_value_double(env, argv[1], &ctr) != napi_ok || !get_u8_array(env, argv[2], &actor, &actor_len) ||
      napi_get_value_double(env, argv[3], &first) != napi_ok || napi_get_value_double(env, argv[4], &n) != napi_ok || ctr < 0 || ctr > 4294967295.0 || first < 0 ||
      n < 0 || first > 9007199254740991.0 || n > 9007199254740991.0) {
    napi_throw_type_error(env, NULL, "textLocate takes a counter, the actor's bytes, a first position and a count");
    return NULL;
  }
  const am355_text_run *runs = NULL;
  uint32_t n_runs = 0;
  uint64_t length = 0;
  int rc = am355_text_locate(ctx, (uint64_t)ctr, actor, actor_len, (uint64_t)first, (uint64_t)n, &runs, &n_runs, &length);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_object(env, &out));
  NAPI_CALL(env, napi_create_double(env, (double)length, &v));
  NAPI_CALL(env, napi_set_named_property(env, out, "length", v));
  NAPI_CALL(env, napi_create_array_with_length(env, n_runs, &runs_js));
  for (uint32_t r = 0; r < n_runs; r++) {
    napi_value o;
    NAPI_CALL(env, napi_create_object(env, &o));
    if (!id_string(env, ctx, runs[r].elem_ctr, runs[r].elem_actor, &v)) { napi_throw_error(env, NULL, "textLocate: a run names an actor outside the table"); return NULL; }
    NAPI_CALL(env, napi_set_named_property(env, o, "elemId", v));
    if (!id_string(env, ctx, runs[r].pred_ctr, runs[r].pred_actor, &v)) { napi_throw_error(env, NULL, "textLocate: a run names an actor outside the table"); return NULL; }
    NAPI_CALL(env, napi_set_named_property(env, o, "pred", v));
    NAPI_CALL(env, napi_create_uint32(env, runs[r].count, &v));
    NAPI_CALL(env, napi_set_named_property(env, o, "count", v));
    NAPI_CALL(env, napi_get_boolean(env, (runs[r].flags & AM355_RUN_COUNTER) != 0, &v));
    NAPI_CALL(env, napi_set_named_property(env, o, "counter", v));
    NAPI_CALL(env, napi_set_element(env, runs_js, r, o));
  }
  NAPI_CALL(env, napi_set_named_property(env, out, "runs", runs_js));
  return out;
}
/* textSplice(ctx, ctr, Uint8Array actor, start, deletions, Uint8Array utf8, Uint32Array valueOff, Uint8Array author, time, Uint8Array message)
 * -> Uint8Array (the binary change; empty: there was nothing to do) = am355_text_splice: the patch is then read with fetchApplyIR */
static napi_value js_text_splice(napi_env env, napi_callback_info info) {
  size_t argc = 10;
  napi_value argv[10];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double ctr = -1, start = -1, deletions = -1, time = 0;
  const uint8_t *actor = NULL, *utf8 = NULL, *author = NULL, *message = NULL;
  size_t actor_len = 0, utf8_len = 0, author_len = 0, message_len = 0, n_off = 0;
  uint32_t *off = NULL;
  if (argc < 10 || napi_get_value_double(env, argv[1], &ctr) != napi_ok || !get_u8_array(env, argv[2], &actor, &actor_len) ||
      napi_get_value_double(env, argv[3], &start) != napi_ok || napi_get_value_double(env, argv[4], &deletions) != napi_ok || !get_u8_array(env, argv[5], &utf8, &utf8_len) ||
      !get_u32_array(env, argv[6], &off, &n_off) || !get_u8_array(env, argv[7], &author, &author_len) || napi_get_value_double(env, argv[8], &time) != napi_ok ||
      !get_u8_array(env, argv[9], &message, &message_len) || ctr < 0 || ctr > 4294967295.0 || start < 0 || deletions < 0 || start > 9007199254740991.0 ||
      deletions > 9007199254740991.0 || n_off < 1 || off[n_off - 1] != utf8_len || message_len > 0xffffffffu || time != (double)(int64_t)time) {
    napi_throw_type_error(env, NULL, "textSplice takes (ctx, counter, actor bytes, start, deletions, utf8, value offsets, author bytes, time, message bytes)");
    return NULL;
  }
  const uint8_t *bytes = NULL;
  size_t len = 0;
  int rc = am355_text_splice(ctx, (uint64_t)ctr, actor, actor_len, (uint64_t)start, (uint64_t)deletions, utf8, off, (uint32_t)(n_off - 1), author, author_len, (int64_t)time,
                             message, (uint32_t)message_len, &bytes, &len);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value ab = copy_to_arraybuffer(env, bytes, len), change;
  if (!ab) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &change));
  return change;
}

/* listLocate(ctx, ctr, Uint8Array actor, first, n) -> { length, runs: [{ elemId, preds: [opId, ...], count, counter }] } = am355_list_locate:
 * the elements [first, first + n) of a plain list as runs of consecutive elemIds; a run of several elements has one pred, which counts up
 * with the elemId; ids as strings */
static napi_value js_list_locate(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5], out, runs_js, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double ctr = -1, first = -1, n = -1;
  const uint8_t *actor = NULL;
  size_t actor_len = 0;
  if (argc < 5 || napi_get_value_double(env, argv[1], &ctr) != napi_ok || !get_u8_array(env, argv[2], &actor, &actor_len) ||
      napi_get_value_double(env, argv[3], &first) != napi_ok || napi_get_value_double(env, argv[4], &n) != napi_ok || ctr < 0 || ctr > 4294967295.0 || first < 0 ||
      n < 0 || first > 9007199254740991.0 || n > 9007199254740991.0) {
    napi_throw_type_error(env, NULL, "listLocate takes a counter, the actor's bytes, a first position and a count");
    return NULL;
  }
  const am355_list_run *runs = NULL;
  const am355_list_pred *preds = NULL;
  uint32_t n_runs = 0, n_preds = 0;
  uint64_t length = 0;
  int rc = am355_list_locate(ctx, (uint64_t)ctr, actor, actor_len, (uint64_t)first, (uint64_t)n, &runs, &n_runs, &preds, &n_preds, &length);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_object(env, &out));
  NAPI_CALL(env, napi_create_double(env, (double)length, &v));
  NAPI_CALL(env, napi_set_named_property(env, out, "length", v));
  NAPI_CALL(env, napi_create_array_with_length(env, n_runs, &runs_js));
  for (uint32_t r = 0; r < n_runs; r++) {
    napi_value o, preds_js;
    NAPI_CALL(env, napi_create_object(env, &o));
    if (!id_string(env, ctx, runs[r].elem_ctr, runs[r].elem_actor, &v)) { napi_throw_error(env, NULL, "listLocate: a run names an actor outside the table"); return NULL; }
    NAPI_CALL(env, napi_set_named_property(env, o, "elemId", v));
    NAPI_CALL(env, napi_create_array_with_length(env, runs[r].pred_num, &preds_js));
    for (uint32_t q = 0; q < runs[r].pred_num; q++) {
      const am355_list_pred *p = &preds[runs[r].pred_first + q];   /* (inside the array: am355_list_locate checks every run) */
      if (!id_string(env, ctx, p->ctr, p->actor, &v)) { napi_throw_error(env, NULL, "listLocate: a pred names an actor outside the table"); return NULL; }
      NAPI_CALL(env, napi_set_element(env, preds_js, q, v));
    }
    NAPI_CALL(env, napi_set_named_property(env, o, "preds", preds_js));
    NAPI_CALL(env, napi_create_uint32(env, runs[r].count, &v));
    NAPI_CALL(env, napi_set_named_property(env, o, "count", v));
    NAPI_CALL(env, napi_get_boolean(env, (runs[r].flags & AM355_RUN_COUNTER) != 0, &v));
    NAPI_CALL(env, napi_set_named_property(env, o, "counter", v));
    NAPI_CALL(env, napi_set_element(env, runs_js, r, o));
  }
  NAPI_CALL(env, napi_set_named_property(env, out, "runs", runs_js));
  return out;
}
/* listSplice(ctx, ctr, Uint8Array actor, start, deletions, Uint32Array values, Uint8Array strings, Uint8Array author, time, Uint8Array message)
 * listSet(ctx, ctr, Uint8Array actor, index, Uint32Array value, Uint8Array strings, Uint8Array author, time, Uint8Array message)
 * -> Uint8Array (the binary change; empty: there was nothing to do) = am355_list_splice / am355_list_set. values: six words per value, the
 * layout of am355_local_value (js/local_change.js flattenValues); the patch is then read with fetchApplyIR */
static napi_value list_edit(napi_env env, napi_callback_info info, bool is_set) {
  size_t argc = 10, want = is_set ? 9 : 10, a = is_set ? 4 : 5;
  napi_value argv[10];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double ctr = -1, start = -1, deletions = 0, time = 0;
  const uint8_t *actor = NULL, *strings = NULL, *author = NULL, *message = NULL;
  size_t actor_len = 0, strings_len = 0, author_len = 0, message_len = 0, n_words = 0;
  uint32_t *words = NULL;
  const size_t vw = sizeof(am355_local_value) / 4;
  if (argc < want || napi_get_value_double(env, argv[1], &ctr) != napi_ok || !get_u8_array(env, argv[2], &actor, &actor_len) ||
      napi_get_value_double(env, argv[3], &start) != napi_ok || (!is_set && napi_get_value_double(env, argv[4], &deletions) != napi_ok) ||
      !get_u32_array(env, argv[a], &words, &n_words) || !get_u8_array(env, argv[a + 1], &strings, &strings_len) || !get_u8_array(env, argv[a + 2], &author, &author_len) ||
      napi_get_value_double(env, argv[a + 3], &time) != napi_ok || !get_u8_array(env, argv[a + 4], &message, &message_len) || ctr < 0 || ctr > 4294967295.0 || start < 0 ||
      deletions < 0 || start > 9007199254740991.0 || deletions > 9007199254740991.0 || n_words % vw || n_words / vw > 0xffffffffu || (is_set && n_words != vw) ||
      strings_len > 0xffffffffu || message_len > 0xffffffffu || time != (double)(int64_t)time) {
    napi_throw_type_error(env, NULL, is_set ? "listSet takes (ctx, counter, actor bytes, index, one value, strings, author bytes, time, message bytes)"
                                            : "listSplice takes (ctx, counter, actor bytes, start, deletions, values, strings, author bytes, time, message bytes)");
    return NULL;
  }
  am355_local_value *values = (am355_local_value *)malloc(n_words ? n_words * 4 : 1);   /* (a copy: the struct holds a 64-bit word) */
  if (!values) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  if (n_words) memcpy(values, words, n_words * 4);
  const uint8_t *bytes = NULL;
  size_t len = 0;
  int rc = is_set ? am355_list_set(ctx, (uint64_t)ctr, actor, actor_len, (uint64_t)start, values, strings, (uint32_t)strings_len, author, author_len, (int64_t)time, message,
                                   (uint32_t)message_len, &bytes, &len)
                  : am355_list_splice(ctx, (uint64_t)ctr, actor, actor_len, (uint64_t)start, (uint64_t)deletions, values, (uint32_t)(n_words / vw), strings,
                                      (uint32_t)strings_len, author, author_len, (int64_t)time, message, (uint32_t)message_len, &bytes, &len);
  free(values);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value ab = copy_to_arraybuffer(env, bytes, len), change;
  if (!ab) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &change));
  return change;
}
static napi_value js_list_splice(napi_env env, napi_callback_info info) { return list_edit(env, info, false); }
static napi_value js_list_set(napi_env env, napi_callback_info info) { return list_edit(env, info, true); }

/* A primitive value of a map record as the patch carries it: { value } (+ datatype for int / uint / float64 / counter / timestamp; type/length
 * word as in the valLen column, columnar.js:300-329). false: a type this binding does not read (bytes, unknown). */
static bool map_value_object(napi_env env, const am355_ir_map *rec, const uint8_t *arena, uint64_t arena_len, napi_value *out) {
  napi_value v;
  const char *datatype = NULL;
  const uint32_t tag = rec->val_tl & 15u, len = rec->val_tl >> 4;
  if (napi_create_object(env, out) != napi_ok) return false;
  if (rec->flags & AM355_MAP_COUNTER) {
    if (napi_create_double(env, (double)rec->counter, &v) != napi_ok) return false;
    datatype = "counter";
  } else if (tag == 0) { if (napi_get_null(env, &v) != napi_ok) return false; }
  else if (tag == 1 || tag == 2) { if (napi_get_boolean(env, tag == 2, &v) != napi_ok) return false; }
  else {
    if ((uint64_t)rec->val_off + len > arena_len) return false;
    const uint8_t *p = arena + rec->val_off;
    if (tag == 3 || tag == 4 || tag == 8 || tag == 9) {
      uint64_t u = 0;
      int shift = 0;
      if (len == 0 || len > 10) return false;
      for (uint32_t k = 0; k < len; k++, shift += 7) u |= (uint64_t)(p[k] & 0x7f) << shift;
      if (tag != 3 && shift < 64 && (p[len - 1] & 0x40)) u |= ~(uint64_t)0 << shift;
      if (napi_create_double(env, tag == 3 ? (double)u : (double)(int64_t)u, &v) != napi_ok) return false;
      datatype = tag == 3 ? "uint" : tag == 4 ? "int" : tag == 8 ? "counter" : "timestamp";
    } else if (tag == 5 && len == 8) {
      double d;
      memcpy(&d, p, 8);
      if (napi_create_double(env, d, &v) != napi_ok) return false;
      datatype = "float64";
    } else if (tag == 6) {
      const size_t skip = len >= 3 && p[0] == 0xef && p[1] == 0xbb && p[2] == 0xbf ? 3 : 0;   /* (TextDecoder drops a leading U+FEFF) */
      if (napi_create_string_utf8(env, (const char *)p + skip, len - skip, &v) != napi_ok) return false;
    } else return false;
  }
  if (napi_set_named_property(env, *out, "value", v) != napi_ok) return false;
  if (datatype) {
    if (napi_create_string_utf8(env, datatype, NAPI_AUTO_LENGTH, &v) != napi_ok || napi_set_named_property(env, *out, "datatype", v) != napi_ok) return false;
  }
  return true;
}

/* mapLocate(ctx, ctr, Uint8Array actor, Uint8Array keys, Uint32Array keyOff) -> [{ counter, child, ids: [opId, ...], values: [value, ...] }] per key =
 * am355_map_locate: the op ids of the key's visible values in ascending order and what they hold ({ value, datatype } / { objectId }); counter /
 * child: of the value the map shows (the last one). _root: ctr 0 and an empty actor. */
static napi_value js_map_locate(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5], out, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double ctr = -1;
  const uint8_t *actor = NULL, *keys = NULL;
  size_t actor_len = 0, keys_len = 0, n_off = 0;
  uint32_t *off = NULL;
  if (argc < 5 || napi_get_value_double(env, argv[1], &ctr) != napi_ok || !get_u8_array(env, argv[2], &actor, &actor_len) || !get_u8_array(env, argv[3], &keys, &keys_len) ||
      !get_u32_array(env, argv[4], &off, &n_off) || ctr < 0 || ctr > 4294967295.0 || n_off < 1 || n_off - 1 > 0xffffffffu || off[0] != 0 || off[n_off - 1] != keys_len) {
    napi_throw_type_error(env, NULL, "mapLocate takes a counter, the actor's bytes, the keys' bytes and their offsets");
    return NULL;
  }
  for (size_t k = 0; k + 1 < n_off; k++)
    if (off[k] > off[k + 1]) { napi_throw_type_error(env, NULL, "mapLocate: key offsets out of order"); return NULL; }
  const am355_map_hit *hits = NULL;
  const am355_ir_map *recs = NULL;
  uint32_t n_recs = 0;
  const uint32_t n = (uint32_t)(n_off - 1);
  int rc = am355_map_locate(ctx, (uint64_t)ctr, actor, actor_len, keys, off, n, &hits, &recs, &n_recs);
  if (rc) return throw_engine(env, ctx, rc);
  const uint8_t *arena = NULL;
  const uint64_t *offsets = NULL;
  uint32_t n_changes = 0;
  rc = am355_get_raw(ctx, &arena, &offsets, &n_changes);
  if (rc) return throw_engine(env, ctx, rc);
  const uint64_t arena_len = offsets ? offsets[n_changes] : 0;
  NAPI_CALL(env, napi_create_array_with_length(env, n, &out));
  for (uint32_t k = 0; k < n; k++) {
    napi_value o, ids, values;
    NAPI_CALL(env, napi_create_object(env, &o));
    NAPI_CALL(env, napi_get_boolean(env, (hits[k].flags & AM355_MAP_COUNTER) != 0, &v));
    NAPI_CALL(env, napi_set_named_property(env, o, "counter", v));
    NAPI_CALL(env, napi_get_boolean(env, (hits[k].flags & AM355_MAP_CHILD) != 0, &v));
    NAPI_CALL(env, napi_set_named_property(env, o, "child", v));
    NAPI_CALL(env, napi_create_array_with_length(env, hits[k].num, &ids));
    NAPI_CALL(env, napi_create_array_with_length(env, hits[k].num, &values));
    for (uint32_t q = 0; q < hits[k].num; q++) {
      const am355_ir_map *rec = &recs[hits[k].first + q];   /* (inside the array: am355_map_locate checks every hit) */
      napi_value id;
      if (!id_string(env, ctx, rec->id_ctr, rec->id_actor, &id)) { napi_throw_error(env, NULL, "mapLocate: a record names an actor outside the table"); return NULL; }
      NAPI_CALL(env, napi_set_element(env, ids, q, id));
      if (rec->flags & AM355_MAP_CHILD) {
        NAPI_CALL(env, napi_create_object(env, &v));
        NAPI_CALL(env, napi_set_named_property(env, v, "objectId", id));
      } else if (!map_value_object(env, rec, arena, arena_len, &v)) { napi_throw_error(env, NULL, "mapLocate: a value this binding does not read (bytes, or outside the arena)"); return NULL; }
      NAPI_CALL(env, napi_set_element(env, values, q, v));
    }
    NAPI_CALL(env, napi_set_named_property(env, o, "ids", ids));
    NAPI_CALL(env, napi_set_named_property(env, o, "values", values));
    NAPI_CALL(env, napi_set_element(env, out, k, o));
  }
  return out;
}

/* mapUpdate(ctx, ctr, Uint8Array actor, Uint32Array ops, Uint8Array strings, Uint32Array values, Uint8Array author, time, Uint8Array message)
 * -> Uint8Array (the binary change; empty: no op came of it) = am355_map_update. ops: six words per op -- kind, key offset, key length, value
 * index, delta low word, delta high word (the layout of am355_map_op); values: six words per value (js/local_change.js flattenValues), their
 * strings in `strings` beside the keys */
static napi_value js_map_update(napi_env env, napi_callback_info info) {
  size_t argc = 9;
  napi_value argv[9];
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double ctr = -1, time = 0;
  const uint8_t *actor = NULL, *strings = NULL, *author = NULL, *message = NULL;
  size_t actor_len = 0, strings_len = 0, author_len = 0, message_len = 0, n_op_words = 0, n_words = 0;
  uint32_t *op_words = NULL, *words = NULL;
  const size_t vw = sizeof(am355_local_value) / 4, ow = sizeof(am355_map_op) / 4;
  if (argc < 9 || napi_get_value_double(env, argv[1], &ctr) != napi_ok || !get_u8_array(env, argv[2], &actor, &actor_len) || !get_u32_array(env, argv[3], &op_words, &n_op_words) ||
      !get_u8_array(env, argv[4], &strings, &strings_len) || !get_u32_array(env, argv[5], &words, &n_words) || !get_u8_array(env, argv[6], &author, &author_len) ||
      napi_get_value_double(env, argv[7], &time) != napi_ok || !get_u8_array(env, argv[8], &message, &message_len) || ctr < 0 || ctr > 4294967295.0 || n_op_words % ow ||
      n_op_words / ow > 0xffffffffu || n_words % vw || n_words / vw > 0xffffffffu || strings_len > 0xffffffffu || message_len > 0xffffffffu || time != (double)(int64_t)time) {
    napi_throw_type_error(env, NULL, "mapUpdate takes (ctx, counter, actor bytes, ops, strings, values, author bytes, time, message bytes)");
    return NULL;
  }
  /* (copies: both structs hold a 64-bit word) */
  am355_map_op *ops = (am355_map_op *)malloc(n_op_words ? n_op_words * 4 : 1);
  am355_local_value *values = (am355_local_value *)malloc(n_words ? n_words * 4 : 1);
  if (!ops || !values) { free(ops); free(values); napi_throw_error(env, NULL, "out of memory"); return NULL; }
  if (n_op_words) memcpy(ops, op_words, n_op_words * 4);
  if (n_words) memcpy(values, words, n_words * 4);
  const uint8_t *bytes = NULL;
  size_t len = 0;
  int rc = am355_map_update(ctx, (uint64_t)ctr, actor, actor_len, ops, (uint32_t)(n_op_words / ow), strings, (uint32_t)strings_len, values, (uint32_t)(n_words / vw), author,
                            author_len, (int64_t)time, message, (uint32_t)message_len, &bytes, &len);
  free(ops);
  free(values);
  if (rc) return throw_engine(env, ctx, rc);
  napi_value ab = copy_to_arraybuffer(env, bytes, len), change;
  if (!ab) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &change));
  return change;
}

/* rankOfActor(ctx, Uint8Array actor) -> the actor's rank in the engine's table, -1 when the state does not know the actor
 * (am355_rank_of_actor). Ranks are renumbered when a new actor arrives: asked per call. */
static napi_value js_rank_of_actor(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2], v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  const uint8_t *actor = NULL;
  size_t actor_len = 0;
  if (argc < 2 || !get_u8_array(env, argv[1], &actor, &actor_len)) {
    napi_throw_type_error(env, NULL, "rankOfActor takes the actor's bytes");
    return NULL;
  }
  uint32_t rank = 0;
  int rc = am355_rank_of_actor(ctx, actor, actor_len, &rank);
  if (rc && rc != AM355_E_ARG) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_double(env, rc ? -1.0 : (double)rank, &v));
  return v;
}
/* textPositions(ctx, ctr, Uint8Array actor, Uint32Array ids) -> { length, words: Uint32Array } = am355_text_position. ids: (counter, actor
 * rank) pairs, rank 0xffffffff for an actor the state does not know; words: (position, status | flags) pairs, AM355_POS_* */
static napi_value js_text_positions(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4], out, v;
  NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  am355_ctx *ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double ctr = -1;
  const uint8_t *actor = NULL;
  size_t actor_len = 0, n_words = 0;
  uint32_t *ids = NULL;
  if (argc < 4 || napi_get_value_double(env, argv[1], &ctr) != napi_ok || !get_u8_array(env, argv[2], &actor, &actor_len) || !get_u32_array(env, argv[3], &ids, &n_words) ||
      ctr < 0 || ctr > 4294967295.0 || (n_words & 1) || n_words / 2 > 0xffffffffu) {
    napi_throw_type_error(env, NULL, "textPositions takes a counter, the actor's bytes and a Uint32Array of (counter, rank) pairs");
    return NULL;
  }
  const am355_elem_pos *pos = NULL;
  uint64_t length = 0;
  int rc = am355_text_position(ctx, (uint64_t)ctr, actor, actor_len, (const am355_elem_id *)ids, (uint32_t)(n_words / 2), &pos, &length);
  if (rc) return throw_engine(env, ctx, rc);
  NAPI_CALL(env, napi_create_object(env, &out));
  NAPI_CALL(env, napi_create_double(env, (double)length, &v));
  NAPI_CALL(env, napi_set_named_property(env, out, "length", v));
  napi_value ab = copy_to_arraybuffer(env, (const uint8_t *)pos, n_words * 4), words;
  if (!ab) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n_words, ab, 0, &words));
  NAPI_CALL(env, napi_set_named_property(env, out, "words", words));
  return out;
}

static napi_value init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"create", NULL, js_create, NULL, NULL, NULL, napi_enumerable, NULL},
      {"destroy", NULL, js_destroy, NULL, NULL, NULL, napi_enumerable, NULL},
      {"loadChanges", NULL, js_load_changes, NULL, NULL, NULL, napi_enumerable, NULL},
      {"loadDocument", NULL, js_load_document, NULL, NULL, NULL, napi_enumerable, NULL},
      {"backendLoad", NULL, js_backend_load, NULL, NULL, NULL, napi_enumerable, NULL},
      {"replay", NULL, js_replay, NULL, NULL, NULL, napi_enumerable, NULL},
      {"patchJSON", NULL, js_patch_json, NULL, NULL, NULL, napi_enumerable, NULL},
      {"save", NULL, js_save, NULL, NULL, NULL, napi_enumerable, NULL},
      {"appliedOrder", NULL, js_applied_order, NULL, NULL, NULL, napi_enumerable, NULL},
      {"appliedInInputOrder", NULL, js_applied_in_input_order, NULL, NULL, NULL, napi_enumerable, NULL},
      {"hashes", NULL, js_hashes, NULL, NULL, NULL, napi_enumerable, NULL},
      {"stats", NULL, js_stats, NULL, NULL, NULL, napi_enumerable, NULL},
      {"docChanges", NULL, js_doc_changes, NULL, NULL, NULL, napi_enumerable, NULL},
      {"fetchIR", NULL, js_fetch_ir, NULL, NULL, NULL, napi_enumerable, NULL},
      {"applyChanges", NULL, js_apply_changes, NULL, NULL, NULL, napi_enumerable, NULL},
      {"pendingOrder", NULL, js_pending_order, NULL, NULL, NULL, napi_enumerable, NULL},
      {"forgetCallHistory", NULL, js_forget_call_history, NULL, NULL, NULL, napi_enumerable, NULL},
      {"hashGraphKnown", NULL, js_hash_graph_known, NULL, NULL, NULL, napi_enumerable, NULL},
      {"reset", NULL, js_reset, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setResidentNewActors", NULL, js_set_resident_new_actors, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setResidentMapMerge", NULL, js_set_resident_map_merge, NULL, NULL, NULL, napi_enumerable, NULL},
      {"residentMapMergeCalls", NULL, js_resident_map_merge_calls, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setResidentNewObjects", NULL, js_set_resident_new_objects, NULL, NULL, NULL, napi_enumerable, NULL},
      {"residentNewObjectCalls", NULL, js_resident_new_object_calls, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setResidentCounters", NULL, js_set_resident_counters, NULL, NULL, NULL, napi_enumerable, NULL},
      {"residentCounterCalls", NULL, js_resident_counter_calls, NULL, NULL, NULL, napi_enumerable, NULL},
      {"depGraph", NULL, js_dep_graph, NULL, NULL, NULL, napi_enumerable, NULL},
      {"findChanges", NULL, js_find_changes, NULL, NULL, NULL, napi_enumerable, NULL},
      {"changesSince", NULL, js_changes_since, NULL, NULL, NULL, napi_enumerable, NULL},
      {"changesAdded", NULL, js_changes_added, NULL, NULL, NULL, napi_enumerable, NULL},
      {"missingDeps", NULL, js_missing_deps, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setGraphProbeMin", NULL, js_set_graph_probe_min, NULL, NULL, NULL, napi_enumerable, NULL},
      {"graphQueryCalls", NULL, js_graph_query_calls, NULL, NULL, NULL, napi_enumerable, NULL},
      {"objectText", NULL, js_object_text, NULL, NULL, NULL, napi_enumerable, NULL},
      {"textLocate", NULL, js_text_locate, NULL, NULL, NULL, napi_enumerable, NULL},
      {"textSplice", NULL, js_text_splice, NULL, NULL, NULL, napi_enumerable, NULL},
      {"listLocate", NULL, js_list_locate, NULL, NULL, NULL, napi_enumerable, NULL},
      {"listSplice", NULL, js_list_splice, NULL, NULL, NULL, napi_enumerable, NULL},
      {"listSet", NULL, js_list_set, NULL, NULL, NULL, napi_enumerable, NULL},
      {"mapLocate", NULL, js_map_locate, NULL, NULL, NULL, napi_enumerable, NULL},
      {"mapUpdate", NULL, js_map_update, NULL, NULL, NULL, napi_enumerable, NULL},
      {"textPositions", NULL, js_text_positions, NULL, NULL, NULL, napi_enumerable, NULL},
      {"rankOfActor", NULL, js_rank_of_actor, NULL, NULL, NULL, napi_enumerable, NULL},
      {"bloomBuild", NULL, js_bloom_build, NULL, NULL, NULL, napi_enumerable, NULL},
      {"bloomProbe", NULL, js_bloom_probe, NULL, NULL, NULL, napi_enumerable, NULL},
      {"fetchApplyIR", NULL, js_fetch_apply_ir, NULL, NULL, NULL, napi_enumerable, NULL},
      {"encodeChange", NULL, js_encode_change, NULL, NULL, NULL, napi_enumerable, NULL},
      {"applyLocalChange", NULL, js_apply_local_change, NULL, NULL, NULL, napi_enumerable, NULL},
      {"localChangeCalls", NULL, js_local_change_calls, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setLocalSmall", NULL, js_set_local_small, NULL, NULL, NULL, napi_enumerable, NULL},
      {"localSmallCalls", NULL, js_local_small_calls, NULL, NULL, NULL, napi_enumerable, NULL},
      {"shardUniqueId", NULL, js_shard_unique_id, NULL, NULL, NULL, napi_enumerable, NULL},
      {"shardInit", NULL, js_shard_init, NULL, NULL, NULL, napi_enumerable, NULL},
      {"shardedReplay", NULL, js_sharded_replay, NULL, NULL, NULL, napi_enumerable, NULL},
      {"shardFragmentBytes", NULL, js_shard_fragment_bytes, NULL, NULL, NULL, napi_enumerable, NULL},
      {"shardFinalize", NULL, js_shard_finalize, NULL, NULL, NULL, napi_enumerable, NULL},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
