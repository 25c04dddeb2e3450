/*
 * am355.h -- C ABI of the MI355X-native bulk change-replay engine for automerge-classic's backend.
 *
 * This is the drop-in boundary for ONE path of the reference: Backend.loadChanges(Backend.init(), changes)
 * followed by Backend.getPatch(state)  (reference: backend/backend.js:116-129, backend/new.js:1797-1879 and
 * 2060-2068; callers: src/automerge.js:52-55 load, :105-118 getHistory, :43-46 clone) -- plus the two calls on
 * either side of it: Backend.load(bytes) (am355_load_document) and Backend.save(state) (am355_save).  The reference is 100 %
 * JavaScript and has no FFI; the host-side binding a maintainer adds is the N-API addon in
 * automerge_classic_amd/js/ (see INTEGRATION.md), which calls exactly these entry points and re-exports the
 * Backend module surface (backend/index.js:1-8) with every other call delegated to the JS backend.
 *
 * Plain pointers and sizes only; no C++ or torch types.  All functions return 0 on success or a negative
 * AM355_E_* code; am355_last_error() gives a message.  A context is bound to one GPU and one HIP stream and
 * is not thread-safe (the reference API is synchronous and single-threaded: backend/columnar.js:8-12); the engine itself
 * uses host threads internally (column DEFLATE in am355_save, patch text in am355_patch_json).
 *
 * The engine has no CPU fallback: without a gfx950 device am355_create() fails.
 */
#ifndef AM355_H
#define AM355_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct am355_ctx am355_ctx;

enum {
  AM355_OK = 0,
  AM355_E_DEVICE = -1,      /* no usable GPU / HIP error */
  AM355_E_ARG = -2,         /* bad argument */
  AM355_E_INVALID = -3,     /* the reference would throw on this input (RangeError); see am355_flags() */
  AM355_E_UNSUPPORTED = -4, /* legal input outside the GPU-served subset; the JS host replays it on the JS path */
  AM355_E_STATE = -5,       /* call sequence error */
  AM355_E_NOMEM = -6
};

/* Validity / support flags (bit set), as raised by the device kernels and the host scheduler. */
enum {
  AM355_F_BAD_MAGIC = 1u << 0, AM355_F_BAD_CHECKSUM = 1u << 1, AM355_F_BAD_CHUNK = 1u << 2, AM355_F_BAD_COLUMNS = 1u << 3,
  AM355_F_BAD_LEB = 1u << 4, AM355_F_BAD_RLE = 1u << 5, AM355_F_BAD_ROW = 1u << 6, AM355_F_UNKNOWN_OBJECT = 1u << 7,
  AM355_F_BAD_ELEM = 1u << 8, AM355_F_BAD_PRED = 1u << 9, AM355_F_DUP_OPID = 1u << 10, AM355_F_BAD_COUNTER = 1u << 11,
  AM355_F_UNSUPPORTED = 1u << 12, AM355_F_OVERFLOW = 1u << 13,
  AM355_F_BAD_SEQ = 1u << 16,        /* new.js:1571-1578 sequence number reuse / gap */
  AM355_F_UNKNOWN_ACTOR = 1u << 17,  /* new.js:1442-1449 */
  AM355_F_BAD_DEFLATE = 1u << 18     /* columnar.js:813-823 inflate failure */
};

am355_ctx *am355_create(int device_ordinal);
void am355_destroy(am355_ctx *ctx);
const char *am355_last_error(const am355_ctx *ctx);
uint32_t am355_flags(const am355_ctx *ctx);

/*
 * Stage a batch of binary changes: `arena` holds n_changes change containers back to back, change i occupying
 * arena[offsets[i] .. offsets[i+1]).  DEFLATEd changes (chunk type 2, columnar.js:798-823) are inflated on the
 * host (libdeflate when the system has it, else zlib) into an internal pinned "raw arena", which is copied to HBM.  Replaces
 * the per-buffer decodeChangeColumns() preamble of BackendDoc.applyChanges (new.js:1806-1810).  The caller's buffers are not
 * retained: when the call returns every byte is in the engine's arena -- the copies to HBM may still be running; am355_replay
 * is ordered behind them on the context's stream (the next load waits for them before it rewrites the arena).
 */
int am355_load_changes(am355_ctx *ctx, const uint8_t *arena, const uint64_t *offsets, uint32_t n_changes);

/*
 * Stage one saved document (chunk type 0, as written by Backend.save / Automerge.save): container + header parse, chunk
 * checksum, zlib inflate of DEFLATEd columns and the change-metadata scan (clock) on the host, op columns to HBM.
 * Replaces decodeDocumentHeader + readDocumentChanges of `new BackendDoc(buffer)` (columnar.js:1006-1038, new.js:1645-1675,
 * 1695-1750).  am355_replay then decodes the op columns and builds the whole-document patch on the device, so
 * am355_load_document + am355_replay + am355_patch_json == JSON.stringify(Backend.getPatch(Backend.load(bytes))).
 */
int am355_load_document(am355_ctx *ctx, const uint8_t *doc, size_t len);

/*
 * Backend.load(bytes) in ONE call (backend/backend.js:104-107 -> new BackendDoc(buffer), new.js:1695-1750) = am355_load_document +
 * am355_replay, with two things the two-call form cannot do: the chunk checksum (columnar.js:699-705, one SHA-256 over the whole
 * document: a dependent chain of ~20 ms for a 44 MB document, longer than everything else of the load) runs on a thread of its own
 * beside the inflate, the copies to HBM AND the device stages, and its verdict is asked for at the end (a mismatch outranks any other
 * finding, as in the reference, which verifies it first); and the copy of the patch IR to host memory is enqueued behind the device
 * stages right away, so that am355_fetch_ir / am355_patch_json find it under way. Same results, errors and flags as the two calls.
 */
int am355_backend_load(am355_ctx *ctx, const uint8_t *doc, size_t len);

/*
 * The hot path, device-resident in and out: container parse + SHA-256 + column decode, causal scheduling
 * (host, between two device phases), op-set merge, RGA ordering, whole-document patch IR.  Equivalent to
 * Backend.loadChanges(Backend.init(), changes) + the work of Backend.getPatch().  Blocking.
 * May be called repeatedly on the same staged batch (each call recomputes everything).
 */
int am355_replay(am355_ctx *ctx);

/* Copy the patch IR to the host (pinned buffers owned by ctx) and render JSON.stringify(Backend.getPatch(state))
 * byte-for-byte.  `*json` is NUL-terminated and valid until the next call on ctx. */
int am355_patch_json(am355_ctx *ctx, const char **json, size_t *len);

/* ---- results / introspection ---- */
typedef struct {
  uint32_t n_changes, n_applied, n_pending;
  uint32_t n_actors, n_objects, n_heads;
  uint64_t n_ops;        /* op rows in applied changes (dels included): the unit of the ops/s metric */
  uint64_t max_op;
  uint64_t raw_bytes;    /* bytes of the staged (uncompressed) changes */
  uint64_t n_map_values, n_list_elems, n_edits;
  uint64_t ir_bytes;     /* bytes of patch IR produced in HBM by the last replay */
  /* timing of the last am355_replay (milliseconds; device figures from HIP events on the engine's stream). ms_parse / ms_decode /
     ms_merge / ms_order are measured only by a context created with AM355_PHASE_EVENTS=1 in the environment (else 0): an event
     record between two kernels is a packet of its own in front of the next dispatch, i.e. microseconds of the replay itself. */
  float ms_total, ms_parse, ms_host_schedule, ms_decode, ms_merge, ms_order;
  float ms_hash_stream;  /* SHA-256 + dependency resolution on the second stream (overlaps decode/merge) */
  uint32_t fast_path;    /* 1: in-order fast path (device-verified); 2: general path, scheduled on the device (csrc/am355_sched.hip);
                            0: general path, scheduled by the host (thousands of actors, pathological dependency chains) */
} am355_stats;
int am355_get_stats(const am355_ctx *ctx, am355_stats *out);
/* Measurement switch: on != 0 makes the following replays record HIP events between their phases (ms_parse / ms_decode / ms_merge /
 * ms_order of am355_stats); 0 (the default, unless AM355_PHASE_EVENTS=1 is in the environment at am355_create) leaves them out of the
 * stream and reports those four as 0. No counterpart in the reference. */
int am355_set_phase_events(am355_ctx *ctx, int on);

/* 32-byte SHA-256 change hashes in input order (columnar.js:693-705). `out` holds 32 * n_changes bytes. */
int am355_get_hashes(const am355_ctx *ctx, uint8_t *out);

/* Input indexes of the applied changes, in application order (what BackendDoc.changes holds, backend/new.js:1847, and
 * Backend.getAllChanges returns, new.js:1924-1927): duplicates and queued changes do not appear. Valid after am355_replay
 * of changes. out may be NULL to query the count. */
int am355_get_applied(const am355_ctx *ctx, uint32_t *out, uint32_t *n_applied);

/* Backend.save(state) (reference: backend/new.js:2033-2055 BackendDoc.save, backend/columnar.js:983-1004
 * encodeDocumentHeader): the document as one binary chunk -- actor table in order of first appearance, heads, change
 * metadata columns, all non-`del` op rows in canonical order with their succ lists (columns encoded on the GPU),
 * columns of >= 256 bytes DEFLATEd. Valid after am355_replay. A state produced by am355_load_document returns the
 * bytes it was loaded from, as the reference does (new.js:2034); flags bit 0 forces a re-encode of its op columns
 * (diagnostic for the column encoders). AM355_E_UNSUPPORTED while changes are queued (the JS path saves those).
 * *bytes is owned by ctx and valid until the next am355_save / am355_destroy. */
int am355_save(am355_ctx *ctx, uint32_t flags, const uint8_t **bytes, size_t *len);

/* History of a loaded document (reference: backend/new.js:1887-1912 BackendDoc.computeHashGraph ->
 * backend/columnar.js:1040-1047 decodeDocument, :876-943 groupChangeOps, :945-981 decodeDocumentChanges, :710-739 encodeChange):
 * the binary changes the document was made of, in document order -- what Backend.getAllChanges(Backend.load(bytes)) returns --
 * and their 32-byte hashes.  The op columns come from the GPU decode of am355_replay; regrouping rows into changes
 * (`del` ops rebuilt from succ lists, preds = inverse of succ), re-encoding each change and chaining the hashes runs on the
 * engine's host threads.  flags bit 0: DEFLATE changes of >= 256 bytes as encodeChange does (columnar.js:738).
 * Valid after am355_load_document + am355_replay.  AM355_E_INVALID when the document's heads do not match the rebuilt hash graph
 * or its rows / change metadata contradict each other (the reference throws); AM355_E_UNSUPPORTED for documents holding what this
 * path does not rebuild byte for byte (child / link columns, byte-array or unknown-typed values, non-minimal numbers, columns
 * outside the modelled set): the JS path serves those.  Pointers are owned by ctx and valid until the next load / destroy. */
int am355_doc_changes(am355_ctx *ctx, uint32_t flags, const uint8_t **arena, const uint64_t **offsets, uint32_t *n_changes,
                      const uint8_t **hashes);

/* Raw (uncompressed) arena as staged by am355_load_changes: pointers valid until the next load. */
int am355_get_raw(const am355_ctx *ctx, const uint8_t **arena, const uint64_t **offsets, uint32_t *n_changes);

/*
 * Patch IR on the host (valid after am355_fetch_ir or am355_patch_json; owned by ctx, pinned memory).  This is the OUTPUT of the
 * hot path: three record tables written by the device in exactly this layout and copied to the host as they are (three copies).
 * The N-API addon hands them to JavaScript as external ArrayBuffers and automerge_classic_amd/js/materialize.js builds the patch
 * object from them; am355_patch_json renders the same tables as JSON text.  Values and map keys are byte ranges of the raw
 * arena; op ids are (counter, actor rank) with the actor table in the envelope.
 *
 *   objects   index 0 is _root, then the make ops in application order.  A map/table object owns the map records
 *             [map_begin, map_end), a list/text object the edit records [edit_begin, edit_end).
 *   map       one record per visible value of a map key (conflicts: several records with the same key), sorted by (object, key in
 *             UTF-16 code unit order, op id)  -- new.js:1035-1039 `props[key][opId] = value`.
 *   edits     the edits of the reference's whole-document patch, in document order: insert, update, or multi-insert (new.js:747-782
 *             appendEdit: consecutive op ids of one actor, elemId == opId, same value class).  A record carries
 *             count = edits[k+1].first - first values (the table ends with a sentinel record whose `first` is n_values), all with
 *             the SAME type/length word, their bytes back to back in the arena from val_off on -- consecutive ops of one change
 *             have consecutive values in its valRaw column, so a typed run is one record and needs no per-value table.  A
 *             multi-insert whose values change length (mixed-width UTF-8) continues in the next record (AM355_EDIT_CONT): the
 *             host appends that record's values to the same edit.  count >= 2 or a following CONT record = multi-insert.
 *             (type/length word as in the valLen column: len << 4 | type, columnar.js:300-329.)
 */
typedef struct {
  uint32_t id_ctr, id_actor;      /* objectId = id_ctr@actor (ignored for _root) */
  uint32_t type;                  /* action of the make op: 0 makeMap, 2 makeList, 4 makeText, 6 makeTable */
  uint32_t map_begin, map_end;    /* map / table: range of map records */
  uint32_t edit_begin, edit_end;  /* list / text: range of edit records */
  uint32_t make_row;              /* (engine-internal: op row of the make op) */
} am355_ir_object;
enum { AM355_MAP_COUNTER = 1u, AM355_MAP_CHILD = 2u,
       AM355_MAP_EMPTY = 4u   /* incremental patches only: the key is left without a value (`props[key] = {}`, new.js:1037) */ };
typedef struct {
  uint32_t id_ctr, id_actor;      /* opId under which the value is listed */
  uint32_t key_off, key_len;      /* key bytes (UTF-8) in the arena */
  uint32_t val_tl, val_off;       /* value; AM355_MAP_CHILD: val_off = object index */
  uint32_t flags, pad;
  int64_t counter;                /* AM355_MAP_COUNTER: the counter's total (new.js:937-967) */
} am355_ir_map;
enum { AM355_EDIT_UPDATE = 1u, AM355_EDIT_CONT = 2u, AM355_EDIT_CHILD = 4u,
       AM355_EDIT_REMOVE = 8u, /* `remove` edit of count = next record's first - first elements (new.js:775-777, 1029): incremental patches, and
                                  whole-document patches of lists that hold a visible row without a value (an increment of a deleted counter) */
       AM355_EDIT_MULTI = 16u, /* incremental patches only: a `multi-insert` edit even with one value left (appendUpdate took the last
                                  value of a two-value multi-insert away, new.js:812-814; the reference keeps the edit's action) */
       AM355_EDIT_COUNTER = 32u /* the value is the total of a counter inside a list (new.js:937-965): one value per record,
                                  (int64_t)((uint64_t)pad << 32 | val_off); val_tl keeps the type/length word of the counter's `set` */ };
typedef struct {
  uint32_t flags;                 /* AM355_EDIT_UPDATE: `update` edit (else insert / multi-insert); AM355_EDIT_CHILD: the value is an object;
                                     AM355_EDIT_CONT: more values of the previous record's multi-insert */
  uint32_t index;                 /* list index (of the record's first value) */
  uint32_t id_ctr, id_actor;      /* opId (of the record's first value) */
  uint32_t elem_ctr, elem_actor;  /* elemId */
  uint32_t first;                 /* ordinal of the record's first value among all list values; count = next record's first - first */
  uint32_t val_tl;                /* type/length word of every value of the record */
  uint32_t val_off;               /* arena offset of the first value (value i at val_off + i * (val_tl >> 4)); AM355_EDIT_CHILD: object index */
  uint32_t pad;                   /* AM355_EDIT_COUNTER: high word of the total */
} am355_ir_edit;

typedef struct {
  uint32_t n_objects, n_map, n_edits, n_values;   /* n_values: visible list values (sum of the records' counts) */
  const am355_ir_object *objects; /* [n_objects] */
  const am355_ir_map *map;        /* [n_map] */
  const am355_ir_edit *edits;     /* [n_edits + 1] (sentinel) */
  /* envelope */
  uint64_t max_op;
  uint32_t n_actors;            /* actors by rank (lexicographic order of raw ids) */
  const uint32_t *actor_off;    /* [n_actors+1] into actor_bytes */
  const uint8_t *actor_bytes;
  uint32_t n_clock;
  const uint32_t *clock_actor;  /* actor rank, in first-applied order (JS property order of `clock`) */
  const uint64_t *clock_seq;
  uint32_t n_heads;
  const uint8_t *heads;         /* 32 bytes each, sorted */
  uint32_t pending;
  const uint8_t *arena;         /* raw arena (values and keys are ranges of it) */
  uint64_t arena_len;
} am355_patch_ir;
int am355_fetch_ir(am355_ctx *ctx, am355_patch_ir *out);

/*
 * Backend.applyChanges(state, changes) with the INCREMENTAL patch it returns (reference: backend/backend.js:27-31,
 * backend/new.js:1797-1879 BackendDoc.applyChanges, :1052-1290 mergeDocChangeOps, :884-1040 updatePatchProperty in its incremental
 * mode, :747-782 appendEdit, :1461-1528 setupPatches).  `state` is what the context holds: the changes of an earlier
 * am355_load_changes + am355_replay or of earlier am355_apply_changes calls (applied and queued ones), or nothing -- then the call
 * is Backend.applyChanges(Backend.init(), changes).  The engine replays the earlier changes and the batch together (the queue
 * semantics of new.js:1822-1841 included) and derives the patch of the batch from the merged state and from which op rows are new
 * (automerge_classic_amd/csrc/am355_delta.hip): list edits with the index they had when the op was applied, the visible values of every map key
 * the batch touched, and the links from the touched objects up to _root.  Afterwards am355_apply_patch_json / am355_fetch_apply_ir
 * give that patch, and am355_patch_json / am355_fetch_ir / am355_save / am355_get_applied ... describe the new state as after
 * am355_replay.
 * AM355_E_INVALID: the reference throws on this batch.  AM355_E_UNSUPPORTED: legal, but outside the subset served here -- the error
 * text names the reason (DR_* in csrc/am355_delta.h): a list element that holds a `link` op, or counter rows on which the reference's
 * count of visible elements and the values it lists part, or more value rows than the stage walks, a deletion whose place in the
 * merge loop's work list is ambiguous, a property history
 * the device cannot replay (too long, or dependent on call boundaries the host did not keep), a sharded context.  A context made by
 * am355_load_document + am355_replay IS served: Backend.applyChanges(Backend.load(doc), changes) -- the engine rebuilds the document's
 * changes (am355_doc_changes: what computeHashGraph does in the reference), replays them as the state the batch goes onto, schedules
 * the batch as a BackendDoc without hash graph does (am355_hash_graph_known) and takes objectMeta from the document's rows; documents
 * am355_doc_changes refuses are refused here with its reason.  Assignments to list elements, conflicting ones included (several values per element: one edit record per
 * visible value), are served.  The host serves a refused call on the JS path.  After either error the context no longer holds a
 * state (every refusal path drops it: load again).
 */
int am355_apply_changes(am355_ctx *ctx, const uint8_t *arena, const uint64_t *offsets, uint32_t n_changes);
/* Forget the state the context holds: the next am355_apply_changes is Backend.applyChanges(Backend.init(), changes). */
int am355_reset(am355_ctx *ctx);
/* The staged changes were NOT applied by the one am355_load_changes + am355_replay that built the state: the host replayed the
 * retained changes of a state that several Backend.applyChanges calls had built (automerge_classic_amd/js/index.js does so when the
 * context of a state has moved on). Where those calls ended is then not known to the engine -- the reference's merge calls never
 * cross a call (new.js:1052-1290 runs per applyChanges), and what its objectMeta.children lists depends on them (new.js:916-931,
 * 1125-1149) --: am355_apply_changes then refuses the few patches that depend on it instead of assuming one call.
 * from_document = n > 0: the first n staged changes are the REBUILT history of a document that the reference loaded (Backend.load):
 * its objectMeta came from one pass over the document's rows (new.js:1604-1635, 1695-1750), not from that history -- the delta stage
 * replays that pass for the properties it must know (am355_delta.hip kh_simulate) --, and whether the reference has rebuilt the
 * document's hash graph by now is unknown unless am355_hash_graph_known says: a batch whose schedule depends on it is refused.
 * Holds until am355_reset / the next am355_load_changes. */
int am355_forget_call_history(am355_ctx *ctx, int from_document);
/* A BackendDoc made by Backend.load knows the hashes of the document's heads only; it rebuilds the hashes of all the document's changes
 * (computeHashGraph, new.js:1887-1912) when an applyChanges call gets stuck on a missing dependency (new.js:1833-1840) or when
 * getChanges / getChangeByHash / getMissingDeps / getChangesAdded / clone / applyLocalChange ask (new.js:1774, 1922, 1980, 2000, 2015,
 * backend.js:38). Until then applyChanges schedules against what it knows, and the call that rebuilds the graph forgets the hashes
 * of the changes it had applied so far -- both show in the patch (`pendingChanges`, `clock`, `deps`) and in the state. am355_apply_changes
 * reproduces that for a context made by am355_load_document (and for the calls that follow); the host, which serves those queries
 * from am355_doc_changes, says here that the reference would have the graph by now.
 * set: 1 = the graph has been rebuilt, 0 = not yet (after am355_forget_call_history(ctx, n)), -1 = only ask. *known (may be NULL):
 * the state after the call -- 1 for every lineage that did not begin with a document. */
int am355_hash_graph_known(am355_ctx *ctx, int set, int *known);

/* Input indexes of the changes still queued for a missing dependency (BackendDoc.queue, new.js:1866), in queue order. The engine's
 * own list of changes after am355_apply_changes is: the changes applied before the call in application order, the batch, the
 * changes queued before the call -- am355_get_applied / am355_get_pending / am355_get_hashes index that list. out may be NULL. */
int am355_get_pending(const am355_ctx *ctx, uint32_t *out, uint32_t *n_pending);
/* JSON.stringify of the patch Backend.applyChanges returned -- byte for byte; valid until the next call on ctx */
int am355_apply_patch_json(am355_ctx *ctx, const char **json, size_t *len);
/* The same patch as record tables (layout above; records may carry AM355_EDIT_REMOVE / AM355_MAP_EMPTY, map records of one object
 * come in the order the reference inserted the keys, objects the patch does not reach have empty ranges). */
int am355_fetch_apply_ir(am355_ctx *ctx, am355_patch_ir *out);

/*
 * Backend.applyLocalChange(state, request) (reference: backend/backend.js:54-91; backend/columnar.js:710-739 encodeChange, :446-475
 * expandMultiOps, :122-170 parseAllOpIds, :370-444 encodeOps). A change REQUEST is what the frontend hands over: ops that still carry
 * `values` / `multiOp`, no hash. Here it is flat -- the bindings fill it (engine.py, js/local_change.js), nothing in C parses JS
 * objects or JSON --, the device expands the ops into rows, gives numbers their bytes and encodes the twelve op columns
 * (am355_hist.hip kl_expand + the encoders of am355_encode.hip); the host writes the container around them and hashes it.
 *
 * Actors are CHANGE-LOCAL numbers: the table holds the author first, then every other actor an op names, in byte order
 * (columnar.js:154-157), each exactly once; actor_rank[i] = position of entry i among all entries in byte order (preds of an op are
 * ordered by counter, then by actor id -- not by local number: compareParsedOpIds). Keys and UTF-8 values are ranges of `strings`.
 */
enum { AM355_LK_STRING = 0, AM355_LK_HEAD = 1, AM355_LK_ELEM = 2 };          /* am355_local_op.key_kind */
enum { AM355_LOP_INSERT = 1u, AM355_LOP_VALUES = 2u };                       /* am355_local_op.flags: `insert` | the op has `values` */
enum { AM355_LV_NULL = 0, AM355_LV_FALSE = 1, AM355_LV_TRUE = 2, AM355_LV_UINT = 3, AM355_LV_INT = 4, AM355_LV_FLOAT64 = 5,
       AM355_LV_UTF8 = 6, AM355_LV_BYTES = 7, AM355_LV_COUNTER = 8, AM355_LV_TIMESTAMP = 9,
       AM355_LV_BAD = 15 /* a value the reference throws on: a bad value / datatype pair of a multi-insert, a number its datatype cannot hold */ };
typedef struct {
  uint32_t action;                 /* index into ACTIONS: 0 makeMap, 1 set, 2 makeList, 3 del, 4 makeText, 5 inc, 6 makeTable */
  uint32_t obj_actor, obj_ctr;     /* obj_actor UINT32_MAX: _root */
  uint32_t key_kind;               /* AM355_LK_* */
  uint32_t key_off, key_len;       /* AM355_LK_STRING */
  uint32_t elem_actor, elem_ctr;   /* AM355_LK_ELEM */
  uint32_t flags;                  /* AM355_LOP_* */
  uint32_t multi;                  /* rows the op expands to: values.length with AM355_LOP_VALUES, multiOp of a `del`, else 1 */
  uint32_t val_first;              /* `set` / `inc`: its value; with AM355_LOP_VALUES the first of `multi` values */
  uint32_t pred_first, pred_num;
} am355_local_op;
typedef struct {
  uint32_t tag;                    /* AM355_LV_* */
  uint32_t off, len;               /* AM355_LV_UTF8: range of `strings` */
  uint32_t pad;
  uint64_t payload;                /* UINT; INT / COUNTER / TIMESTAMP (two's complement); FLOAT64 (the IEEE 754 bits) */
} am355_local_value;
typedef struct { uint32_t actor, ctr; } am355_local_pred;
typedef struct {
  uint64_t seq, start_op;
  int64_t time;
  const uint8_t *message; uint32_t message_len;   /* UTF-8, may be empty */
  const uint8_t *deps; uint32_t n_deps;           /* 32 bytes each, any order: the frontend's (other actors' heads) */
  uint32_t n_actors;                              /* >= 1; entry 0 is the author */
  const uint32_t *actor_off;                      /* [n_actors + 1] into actor_bytes (raw bytes, not hex) */
  const uint8_t *actor_bytes;
  const uint32_t *actor_rank;                     /* [n_actors] */
  const uint8_t *strings; uint32_t strings_len;
  const am355_local_op *ops; uint32_t n_ops;
  const am355_local_value *values; uint32_t n_values;
  const am355_local_pred *preds; uint32_t n_preds;
  uint32_t not_flat;   /* != 0: the request holds what this form cannot express (child / link ops, numeric actions or datatypes, extraBytes,
                          a `hash` field ...): refused with AM355_E_UNSUPPORTED like what the engine itself does not serve */
} am355_local_change;
/*
 * am355_encode_change: encodeChange(request) with the deps as given -- nothing of the context's state is read or touched. *bytes is the
 * binary change as encodeChange returns it (DEFLATEd from 256 bytes on), owned by ctx, valid until the next of these two calls.
 * am355_apply_local_change: backend.js:54-91 -- the seq check; for seq > 1 the author's last hash joins the deps; encode; the
 * one-change batch goes through am355_apply_changes (as the uncompressed container) with the local flag; *change as above. Afterwards
 * am355_apply_patch_json / am355_fetch_apply_ir give the patch applyLocalChange returned.
 * AM355_E_INVALID: the reference throws (a multi-insert with a pred, a multiOp deletion without exactly one pred, a bad value /
 * datatype pair, a seq already applied, no change of the author with seq - 1). AM355_E_UNSUPPORTED: not_flat, byte-array values,
 * unknown actions or value tags, an op of more than 4096 preds, counters beyond 2^31, changes still queued in the state, a sharded
 * context. Both are decided before anything of the state is touched (a document context is at most turned into the state of its
 * rebuilt changes, as am355_apply_changes does); the JS host runs the reference on a refused request, so the exception is the
 * reference's own. A refusal of the apply path itself drops the state as am355_apply_changes does; so does a change that did not
 * apply because a dependency is missing (the reference throws behind the apply then).
 * A lineage that began with a document: the reference rebuilds the document's hash graph when the author's last hash is not among
 * the changes applied since the load (hashByActor, backend.js:34-45) -- the call does what am355_hash_graph_known(ctx, 1) does at
 * exactly that point, and refuses where the host replayed retained changes and the engine cannot tell (am355_forget_call_history).
 * am355_local_change_calls: out[0] requests am355_apply_local_change served, out[1] requests it refused (whatever the code);
 * am355_encode_change applies nothing and is not counted.
 */
int am355_encode_change(am355_ctx *ctx, const am355_local_change *request, const uint8_t **bytes, size_t *len, uint8_t hash[32]);
int am355_apply_local_change(am355_ctx *ctx, const am355_local_change *request, const uint8_t **change, size_t *len);
int am355_local_change_calls(const am355_ctx *ctx, uint64_t out[2]);
/*
 * am355_set_local_small (off by default; with it off both calls above enqueue what they did before the switch existed): on != 0: a
 * request of at most 256 ops that expands to at most 512 rows and 512 pred entries and holds at most 4096 key + value bytes (a key once
 * per row it stands on, 8 bytes per number, a string's UTF-8 length) -- a keystroke, a pasted line -- is built by ONE workgroup: scans,
 * expansion, value bytes and the twelve column encodes in LDS, the columns, their lengths and a flag word written straight into pinned
 * host memory (the upload, one launch, one wait, against ~115 stream commands). The limits are compile-time constants
 * (csrc/am355_hist.h LOCAL_SMALL_OPS / _ROWS / _PREDS / _BYTES) and are checked before anything is enqueued; a request beyond any of them
 * takes the bulk path exactly as with the switch off. Which requests are refused, the change bytes, the hash and the apply half of
 * am355_apply_local_change do not depend on the switch.
 * am355_local_small_calls: out[0] changes the one workgroup built (am355_encode_change counts here too), out[1] requests that found the
 * switch on but lay outside the limits and took the bulk path. Both stay 0 with the switch off.
 * AM355_LOCAL_SMALL_VERIFY=1 in the environment (tests; read per call): after a small build the same request is built again by the bulk
 * path and the twelve lengths and column bytes are compared; a difference is AM355_E_DEVICE with the column named in am355_last_error.
 */
int am355_set_local_small(am355_ctx *ctx, int on);
int am355_local_small_calls(const am355_ctx *ctx, uint64_t out[2]);
/* What the patch of am355_apply_local_change carries beyond the record tables of am355_fetch_apply_ir (whose layout stays as it is):
 * `actor` and `seq` behind `diffs` (new.js:1874-1877). The tables' `heads` are already without the new change's own hash
 * (backend.js:88-89). is_local == 0 when the last patch came from am355_apply_changes. Valid when am355_fetch_apply_ir is. */
typedef struct {
  uint32_t is_local;
  uint32_t actor;   /* actor rank (am355_patch_ir.actor_off / actor_bytes) */
  uint64_t seq;
} am355_local_envelope;
int am355_apply_local_envelope(const am355_ctx *ctx, am355_local_envelope *out);

/*
 * Sync protocol, bulk side (reference backend/sync.js).  A sync message that carries changes is served by
 * am355_apply_changes; what the protocol computes around it over the hashes of a replayed state:
 *   am355_get_dep_graph     the dependency graph of the context's list of changes by index (change i depends on
 *                           dep_index[dep_first[i] .. dep_first[i + 1]); UINT32_MAX: a change the context does not hold) -- what
 *                           BackendDoc.getChanges / getMissingDeps walk (new.js:1921-1976, 2014-2028), resolved on the device while
 *                           the changes were hashed; the pointers are owned by ctx and valid until the next replay
 *   am355_sync_bloom_build  the Bloom filter over the hashes of the changes idx[0 .. n) (sync.js:38-128 BloomFilter of makeBloomFilter,
 *                           :240-244: 10 bits per entry, 7 probes, triple hashing over the first 12 bytes), built on the device from the
 *                           resident hashes; bits receives ceil(n * 10 / 8) bytes (the `bits` field of the filter)
 *   am355_sync_bloom_probe  for a filter received from a peer: contains[k] = 1 iff the hash of change idx[k] is in it
 *                           (BloomFilter.containsHash of getChangesToSend, sync.js:262-283)
 * Valid after am355_replay / am355_apply_changes of changes.
 */
int am355_get_dep_graph(am355_ctx *ctx, const uint32_t **dep_first, const uint32_t **dep_index, uint32_t *n_changes);
int am355_sync_bloom_build(am355_ctx *ctx, const uint32_t *idx, uint32_t n, uint8_t *bits, size_t capacity);
int am355_sync_bloom_probe(am355_ctx *ctx, const uint32_t *idx, uint32_t n, uint32_t num_entries, uint32_t bits_per_entry, uint32_t num_probes,
                           const uint8_t *bits, size_t n_bytes, uint8_t *contains);

/*
 * objectId sharding over several GPUs (one context per GPU, one process per GPU).  Ordering and pred / succ
 * resolution never cross objects (new.js:1141-1145, 1173-1176), so after am355_set_shard(ctx, rank, world) a replay merges
 * only the objects rank `rank` owns (_root: rank 0; any other object: (counter + actor rank) mod world) -- every rank still
 * stages and decodes the whole batch, which keeps op id -> row arithmetic and the object table identical everywhere; the one
 * cross-object link (make op -> child object, new.js:894-897, 973-976) is the object index.  The OUTPUT is what is exchanged:
 * am355_export_fragment writes this rank's record tables as one contiguous block into caller memory (device memory for an
 * RCCL all_gather over xGMI, or host memory), and am355_import_fragments stitches the blocks of all ranks into the patch IR
 * of the whole document, which am355_patch_json / am355_fetch_ir of that context then return.  world == 1 restores the
 * unsharded engine.  am355_save is not available on a sharded context.
 */
int am355_set_shard(am355_ctx *ctx, uint32_t rank, uint32_t world);
int am355_fragment_size(am355_ctx *ctx, size_t *bytes);
int am355_export_fragment(am355_ctx *ctx, void *dst, size_t capacity, int dst_is_device, size_t *len);
/* fragments of ranks 0..world-1 back to back in host memory, fragment r = frags[offsets[r] .. offsets[r+1]) */
int am355_import_fragments(am355_ctx *ctx, const uint8_t *frags, const uint64_t *offsets, uint32_t world);

/*
 * The sharded replay with its collective INSIDE the library: RCCL over xGMI, one process per GPU (north_star: "Changes shard by
 * objectId across the 8 GPUs of one node with an RCCL ... over xGMI").  The library opens librccl.so.1 when the first communicator
 * is made (AM355_RCCL_LIB overrides the name; nothing of RCCL is loaded by a single-GPU user) and calls ncclGetUniqueId /
 * ncclCommInitRank / ncclAllGather / ncclCommDestroy on the context's stream.
 *   am355_shard_unique_id   rank 0 makes the 128-byte id (ncclGetUniqueId); the host carries it to the other ranks' processes
 *                           (the JS host: process.send between the per-GPU workers, js/sharded.js).
 *   am355_shard_init        ncclCommInitRank on the context's GPU; implies am355_set_shard(ctx, rank, world).
 *   am355_sharded_replay    am355_replay of the staged batch (every rank stages the same batch) + one ncclAllGather of
 *                           {failed, fragment bytes} + one ncclAllGather of the patch-IR fragments, HBM to HBM + the stitch
 *                           (am355_import_fragments) on rank 0, or on every rank when stitch_on_all_ranks != 0.  A batch any rank
 *                           rejects is rejected on every rank (no rank waits in a collective).  Afterwards am355_patch_json /
 *                           am355_fetch_ir of a stitching rank return the patch of the WHOLE document.
 *   am355_shard_fragment_bytes  bytes every rank contributed to the last sharded replay (diagnostics, world entries).
 *   am355_shard_finalize    ncclCommDestroy; the context is unsharded again.
 * What the reference has in this place: nothing (a BackendDoc is one single-threaded object, new.js:1695); the partition is legal
 * because preds never cross objects (new.js:1141-1145, 1173-1176) and the one cross-object link is make op -> child (:894-897).
 */
#define AM355_SHARD_ID_BYTES 128
int am355_shard_unique_id(uint8_t id[AM355_SHARD_ID_BYTES]);
int am355_shard_init(am355_ctx *ctx, const uint8_t id[AM355_SHARD_ID_BYTES], uint32_t rank, uint32_t world);
int am355_sharded_replay(am355_ctx *ctx, int stitch_on_all_ranks);
int am355_shard_fragment_bytes(am355_ctx *ctx, uint64_t *bytes, uint32_t capacity);
int am355_shard_finalize(am355_ctx *ctx);

/* diagnostics: how many am355_apply_changes calls on this context merged the batch alone into the resident state (out[0]), how
 * many took the full replay although they asked for it (out[1]: new actor, dependency not applied yet, duplicate, capacity ...), and
 * how many of the first kind also merged their new list elements into the stored document order in place (out[2]) */
int am355_resident_counters(const am355_ctx *ctx, uint64_t out[3]);
/* ... and for how many of the first kind the map half of the merge ran on its own: batches of plain map rows only (`set` / `del` on
 * string keys: every list stayed as it was) and batches of such rows beside list edits (the list rows merged in place first) (*out) */
int am355_resident_maps_only_calls(const am355_ctx *ctx, uint64_t *out);
/* The first changes of a NEW actor on the resident state. The engine stores actor fields as lexicographic ranks, so an actor the
 * document does not know yet renumbers the ranks of the kept rows: by default such a batch takes the full replay ("new actor" among the
 * reasons of am355_resident_counters out[1]), whose cost grows with the document. on != 0: the new authors of the batch are inserted into
 * the sorted actor table and one streaming kernel rewrites the rank words the kept state holds (the actor columns of the op rows and
 * preds, the op ids in the object and map tables, the counters' last increments) in front of the batch's decode -- a monotone
 * renumbering: no order between kept rows changes --; the rest of the call runs as for known actors. An actor id that a change names
 * without anybody in the document or earlier in the batch having authored a change under it still takes the full replay. Off by default;
 * no environment variable. What the reference has in this place: it appends the actor to the document's table and touches no stored op
 * (new.js:1434-1451), because its op ids carry actor indexes in order of first appearance and compare through the id strings.
 * am355_resident_new_actor_calls: calls served on the resident state that inserted at least one actor (out[0]), and how many of those
 * launched the rank rewrite because some kept rank moved (out[1]: an actor that sorts behind every known one moves none). */
int am355_set_resident_new_actors(am355_ctx *ctx, int on);
int am355_resident_new_actor_calls(const am355_ctx *ctx, uint64_t out[2]);
/* Plain map rows (`set` of a value / `del` on a string key: no object made, no increment) merged into the STORED map records. By default
 * a resident call with such rows runs the map half of the merge over the whole document (am355_resident_maps_only_calls: every op row
 * judged again, every map value ordered again), and a document without any list takes all of merge_run: both grow with the document.
 * on != 0: every map row of the batch finds its key's records in the stored table by binary search; the records whose rows the batch
 * overwrote or deleted go out, the batch's visible rows come in -- ordered among themselves --, and one streaming pass writes the merged
 * table beside the stored one and rewrites the objects' map ranges. No pass over the document's op rows, no sort of the stored values.
 * The patch tables are byte for byte what the path of before writes (AM355_MAPMERGE_VERIFY=1 in the environment: every such call
 * rebuilds them that way and compares). Left to the path of before, on state the attempt did not touch: a key that holds more than 256
 * stored values, a batch of more than 16384 rows, declined before anything is enqueued for it (both counted in out[1]); and, as before, batches that increment counters or make
 * objects, which this path does not look at. Off by default; no environment variable. What the reference has in this place:
 * mergeDocChangeOps merges the batch into the stored op set and touches only the blocks it visits (new.js:1052-1290).
 * am355_resident_map_merge_calls: resident calls whose map rows were merged into the stored table in place (out[0]); calls that tried
 * and declined, and were served by the path of before (out[1]). */
int am355_set_resident_map_merge(am355_ctx *ctx, int on);
int am355_resident_map_merge_calls(const am355_ctx *ctx, uint64_t out[2]);
/* Batches that MAKE objects (`doc.cards.push({...})`: a list insert with makeMap and the `set`s inside the new map; `doc.notes = new
 * Text('...')`: a makeText on a key and inserts into the new object) merged into the resident state in place. By default such a batch
 * runs every kernel of merge_run over every row of the document: every list ranked anew, every table rebuilt. on != 0: one pass over the
 * batch's rows gives the objects it makes the next indexes of the stored object table -- the table is in row order of the make rows and
 * the batch's rows stand behind all kept rows, so nothing kept is renumbered -- and the next first positions of the stored list order,
 * which is grouped by object index: the elements of a new object land at its END and no kept object moves because of them. A list
 * insert that makes an object is then a list element like any other, and a make on a string key and the `set` / `del` rows inside maps
 * (new ones too) stand like plain map rows: the list rows are merged into the stored order, the map half of the merge runs behind them
 * (by merge_run_maps also where am355_set_resident_map_merge is on: its stored records do not take makes). Left to merge_run as before
 * (out[1]): a list element ASSIGNED an object (`list[3] = {}`), any `inc` or `link` row in the batch, a make row that names no valid
 * object, and what the in-place list merge declines anyway (a new element with two new children, a gap scan past its limit, more chunks
 * than the path takes). A document without any list element never tries. AM355_RESORDER_VERIFY=1 in the environment: the next rebuild of
 * the whole-document tables compares every object's id, type, make row, first position and element count with what these calls left.
 * Off by default; no environment variable. What the reference has in this place: mergeDocChangeOps inserts the ops into the blocks it
 * visits and updates objectMeta for a make op (new.js:1052-1290, 1118-1131).
 * am355_resident_new_object_calls: resident calls whose batch made at least one object and was served without merge_run (out[0]);
 * calls with the switch on whose batch made an object, were tried in place, were declined and went on with merge_run (out[1]). */
int am355_set_resident_new_objects(am355_ctx *ctx, int on);
int am355_resident_new_object_calls(const am355_ctx *ctx, uint64_t out[2]);
/* Increments of map counters (`doc.votes.increment()`: an `inc` row on a string key) written into the STORED map records in place. By
 * default any `inc` row refuses the in-place stages above and the call runs merge_run over every row of the document. on != 0: such a
 * row takes no part in the list order -- the rest of the batch is merged in place as before --, and one launch over the batch (a
 * wavefront per row) finds the counter every increment feeds among its preds, the counter's object's stretch of the stored map table,
 * the key's records by binary search, and rewrites the counter's record (total = value + increments, the counter flag) where the key
 * holds that one record. Nothing is written for a counter that has no record (deleted or overwritten: it emits nothing before or
 * after). Declined (out[1]) and served by the map half of the merge over the whole document: a key that holds conflicting values (the
 * counter's record stands under its last increment's id and may have to move among them), an increment with more than one pred, a
 * counter made in the same batch. A batch
 * that also holds plain map rows or makes objects runs the map half anyway, which serves its increments too: counted in neither word.
 * Left to merge_run as before: an `inc` on a list element, and -- the list stage never runs there -- a document without any list
 * element. AM355_COUNTERS_VERIFY=1 in the environment: behind every call served, the map table and ranges are rebuilt by the map half
 * and compared byte for byte. Off by default; no environment variable. What the reference has in this place: mergeDocChangeOps visits
 * the block of the counter and adds the increment to its succ list (new.js:1052-1290, 937-965).
 * am355_resident_counter_calls: resident calls whose increments were written into the stored map records in place, with no merge_run and
 * no map half (out[0]); calls where the stage tried and declined (out[1]). */
int am355_set_resident_counters(am355_ctx *ctx, int on);
int am355_resident_counter_calls(const am355_ctx *ctx, uint64_t out[2]);

/* For bindings that mirror per-state tables of the context in their own memory (the N-API addon: BackendDoc.changes, their hashes and
 * the raw arena, backend/new.js:1847, 1855-1879) and must not copy all of them for every one-change Backend.applyChanges:
 *  - am355_arena_epoch: a counter that changes whenever bytes the context handed out as am355_patch_ir.arena may no longer be what
 *    they were (a new am355_load_changes / am355_load_document / am355_reset); while it stays the same the arena has only GROWN at its
 *    end (am355_apply_changes stages a batch behind the kept changes), so a mirror copies [its length, arena_len) only;
 *  - am355_get_hashes_range: change hashes [first, first + count) in input order, 32 bytes each;
 *  - am355_applied_in_input_order: *yes = 1 when every staged change is applied, in the order it was staged, and none is queued (the
 *    applied order is then 0 .. n_changes - 1 and the pending list empty: no need to fetch either). */
int am355_arena_epoch(const am355_ctx *ctx, uint64_t *epoch);
int am355_get_hashes_range(const am355_ctx *ctx, uint32_t first, uint32_t count, uint8_t *out);
int am355_applied_in_input_order(const am355_ctx *ctx, int *yes);

/*
 * Hash-graph queries over the changes the context has APPLIED: what BackendDoc answers from changeIndexByHash, dependenciesByHash
 * and dependentsByHash (new.js:1921-2028), without a BackendDoc. Hashes are 32 raw bytes each. Every index is an index into the
 * context's list of changes -- the list am355_get_applied indexes --; result arrays are owned by the context and valid until the next
 * call on it. The context must hold a replayed state of changes: a document context (am355_load_document) and a context without a
 * replay return AM355_E_STATE, a sharded one AM355_E_UNSUPPORTED, and are left as they were. No call changes the state, the patch
 * tables or what a following am355_apply_changes is served by. Whether the reference would have had to rebuild a loaded document's
 * hash graph for the query stays the caller's business (am355_hash_graph_known).
 *   am355_find_changes   getChangeByHash (new.js:1999-2002): out_idx[k] = the applied change with hash hashes[k], or 0xffffffff.
 *                        A change that is queued for a missing dependency does not count.
 *   am355_changes_since  getChanges(haveDeps) (new.js:1921-1976), in the order the reference returns the changes: forward over the
 *                        dependents of `have`, or -- when that walk meets a change with a dependency it has not seen, or misses a
 *                        head -- every applied change that is not an ancestor of `have`, in application order. n_have == 0: every
 *                        applied change in application order. A hash that is not an applied change: AM355_E_INVALID with the
 *                        text `hash not found: <hex>` (the first such hash of `have`).
 *   am355_changes_added  BackendDoc(ctx).getChangesAdded(other) (new.js:1979-1997): `other` = the hashes of the changes the other
 *                        state has applied, in any order; the result is the depth-first order from the heads through the
 *                        dependencies, stopped at what `other` holds, reversed.
 *   am355_missing_deps   getMissingDeps(heads) (new.js:2014-2028): the dependencies of the queued changes (read from the staged
 *                        bytes) and the given heads that are neither applied nor queued, each once, sorted.
 * The traversals run on the host over indexes. The membership tests -- which of these hashes are applied changes; which changes of
 * the context are missing from `other` -- are answered by a host index, or, from am355_set_graph_probe_min probes on, on the device:
 * a table over the context's hashes, which are in device memory already (find_changes, changes_since, missing_deps: one probe per
 * hash given), or a table over `other` probed with every change of the context, whose answers come back as one bit per change
 * (changes_added: probes = the context's changes). Both give the same result. The default is 65536 probes: the measured crossover of
 * changes_added (between 32,000 and 100,000 changes, profiles/hash_graph_timings.txt) rounded up to a power of two; 0xffffffff: never
 * on the device. am355_graph_query_calls: membership tests answered on the device
 * (out[0]) and by the host index (out[1]); calls that needed none (empty inputs) count in neither.
 */
int am355_find_changes(am355_ctx *ctx, const uint8_t *hashes, uint32_t n, uint32_t *out_idx);
int am355_changes_since(am355_ctx *ctx, const uint8_t *have, uint32_t n_have, const uint32_t **idx, uint32_t *n);
int am355_changes_added(am355_ctx *ctx, const uint8_t *other, uint32_t n_other, const uint32_t **idx, uint32_t *n);
int am355_missing_deps(am355_ctx *ctx, const uint8_t *heads, uint32_t n_heads, const uint8_t **hashes, uint32_t *n);
int am355_set_graph_probe_min(am355_ctx *ctx, uint32_t n);
int am355_graph_query_calls(const am355_ctx *ctx, uint64_t out[2]);

/*
 * The string of a Text object, read on the device from the whole-document edit records (csrc/am355_text.hip): *utf8 / *len are the
 * bytes of exactly the string the reference's frontend shows for that object -- Text.toString() after applyPatch(getPatch(state)) --
 * without the patch being fetched, rendered or applied. The buffer is pinned memory owned by the context, grown on demand and valid
 * until the next call on ctx. The object is named as in the patch: obj_ctr @ the actor's raw bytes.
 * The rule (frontend/apply_patch.js:231-255 updateTextObject, frontend/text.js:64-67 toString):
 *   1. one element per list index;
 *   2. where an element shows several values (its insert plus updates, or updates only behind a row without a value), the last
 *      `update` of that index wins (apply_patch.js:247-250);
 *   3. only values of type UTF8 (val_tl & 15 == 6, columnar.js:47-48) are concatenated (text.js:64-67);
 *   4. numbers, booleans, null, bytes, child objects (AM355_EDIT_CHILD), counter totals (AM355_EDIT_COUNTER) and `remove` records
 *      (AM355_EDIT_REMOVE) contribute nothing;
 *   5. every such element except a `remove` record still counts in the length.
 * A value whose bytes begin EF BB BF contributes without those three bytes: the reference decodes every value by itself with
 * TextDecoder('utf-8'), which drops a leading U+FEFF (encoding.js:9-17). All other bytes are copied as stored: invalid UTF-8 inside a
 * hand-made change is the caller's to decode.
 * info (may be NULL): n_elements = the object's list length (the frontend's text.length), n_strings = the elements whose value is a
 * string, bytes = *len.
 * Served: a state made by am355_replay, a state after am355_apply_changes / am355_apply_local_change (edit tables that in-place
 * merges left stale are rebuilt once, as am355_save does), a document context (am355_backend_load, am355_load_document +
 * am355_replay). The read changes neither the state nor what the next am355_apply_changes is served by, and it leaves the host
 * copies of the tables as they were.
 * AM355_E_STATE: no replayed state. AM355_E_UNSUPPORTED: a sharded context; a typed run of more than 4096 values with values that
 * begin with U+FEFF inside it (read it through the patch). AM355_E_ARG: the id names no object ("no such object: <ctr>@<hex>") or
 * an object that is no Text ("not a Text object"; _root is obj_ctr 0 with actor_len 0). A state whose whole-document patch the engine
 * refuses returns that refusal. AM355_E_DEVICE: a record names values outside the tables (nothing is read or written out of range).
 * am355_object_text_calls: out[0] = calls served, out[1] = kernel launches they made (the library scan counts as one; an empty
 * Text launches nothing beyond the object lookup, which the host's copy of the object table serves when it is current).
 * am355_set_text_pinned_max: strings of up to `bytes` bytes are gathered straight into the pinned buffer instead of into device
 * memory and copied (0 = never). The default is 1 MiB: the direct write was 3-7 us ahead at every size measured, 64 B to 1 MiB
 * (profiles/text_read_timings.txt); longer strings, which were not measured, take the copy.
 * am355_text_limits: the sizes at which the kernels take another path (tests): out[0] = output bytes one workgroup of the gather
 * owns, out[1] = records one workgroup of the size pass takes, out[2] = values of a record its own thread looks at for U+FEFF (more:
 * the workgroup does), out[3] = values of a run with U+FEFF values inside that the gather walks (more: AM355_E_UNSUPPORTED).
 */
typedef struct { uint32_t n_elements, n_strings; uint64_t bytes; } am355_text_info;
int am355_object_text(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len,
                      const uint8_t **utf8, size_t *len, am355_text_info *info /* may be NULL */);
int am355_object_text_calls(const am355_ctx *ctx, uint64_t out[2]);   /* served | device launches made */
int am355_set_text_pinned_max(am355_ctx *ctx, uint64_t bytes);
int am355_text_limits(uint32_t out[4]);

/*
 * A Text edited by POSITION (csrc/am355_locate.hip): the inverse of am355_object_text. A change request names list elements by elemId
 * and a deleted value by its op id (`pred`); a host that keeps a Text on the engine and has no frontend document knows positions only.
 * am355_text_locate resolves the elements [first, first + n) of a Text to their ids on the device, compressed into the runs the
 * reference's frontend would merge into `multiOp` deletions (frontend/context.js:474-492): run = `count` elements whose elemIds are
 * (elem_ctr + i, elem_actor) and whose preds are (pred_ctr + i, pred_actor), i = 0 .. count - 1. Actors are ranks, as in am355_patch_ir.
 * The pred of a Text element is the op id of the last edit of its index (frontend/apply_patch.js:231-255: insert -> opId, multi-insert
 * -> the elemId, update -> opId with the elemId kept). flags & AM355_RUN_COUNTER: some element of the run is a Counter. *runs is pinned
 * memory owned by the context, valid until the next call on ctx; *length = the Text's length (text.length). n == 0 is legal and returns
 * the length. It reads only: the state, what serves the next am355_apply_changes and the host copies of the tables stay as they were
 * (edit tables that in-place merges left stale are rebuilt once, as for am355_object_text). Same contexts and errors as
 * am355_object_text (AM355_E_STATE, sharded AM355_E_UNSUPPORTED, AM355_E_ARG "no such object: ..." / "not a Text object"); first + n >
 * length: AM355_E_ARG; a Text element that shows rows but no value (a `remove` record: an increment of a deleted counter):
 * AM355_E_UNSUPPORTED; records that contradict each other: AM355_E_DEVICE (nothing is read or written out of range).
 *
 * am355_text_splice: one context.splice(path, start, deletions, insertions) of the reference's frontend (context.js:441-502; what
 * text.deleteAt / text.insertAt come down to) on the Text the context holds: it locates [start - 1, start + deletions) in one query,
 * builds exactly the change request the frontend would hand to Backend.applyLocalChange -- one `del` op per run of the deleted elements
 * (multiOp = count), then the insertion behind element start - 1 (`_head` for start == 0): one `set` with `values` for several strings,
 * a plain inserting `set` for one --, with seq = the author's clock entry + 1, startOp = maxOp + 1 and deps = the state's heads without
 * the author's last change, and applies it through am355_apply_local_change (small path, bulk path, patch and envelope as there:
 * am355_apply_patch_json / am355_fetch_apply_ir / am355_apply_local_envelope give the patch). Value i is the UTF-8 string
 * utf8[value_off[i] .. value_off[i + 1]): one list element each. *change / *len: the binary change, as am355_apply_local_change returns
 * it. The caller owns the author and the order of its calls: this path is for hosts WITHOUT a frontend document.
 * Decided before the state is touched (a document context is at most turned into the state of its rebuilt changes): start > length -
 * deletions: AM355_E_ARG with the reference's RangeError text ("<deletions> deletions starting at index <start> are out of bounds for
 * list of length <length>"); a Counter among the deleted elements: AM355_E_INVALID with its TypeError text ("Unsupported operation:
 * deleting a counter from a list"); deletions == 0 && n_values == 0: AM355_OK, *len = 0, nothing applied; the errors of
 * am355_text_locate; queued changes in the state: AM355_E_UNSUPPORTED. What am355_apply_local_change refuses stays refused with its code.
 * am355_text_splice_calls: out[0] splices served, out[1] refused (whatever the code), out[2] kernel launches of the locate half of both
 * calls (the library scan counts as one). am355_text_locate_limits: the sizes at which the kernels take another path (tests): out[0] =
 * elements one workgroup of the locate kernel takes, out[1] = elements up to which the scan of the head bits is one workgroup, out[2] =
 * runs written straight into pinned memory (the ones behind go to device memory and down in one copy).
 * A COUNTER INSIDE A TEXT: context.js:455-471 throws for a counter in a list; for a Text the reference's frontend looks the element up
 * as object[index], which a Text does not have, does not throw and deletes the counter. am355_text_splice refuses as stated above.
 */
enum { AM355_RUN_COUNTER = 1u };                                           /* am355_text_run.flags */
typedef struct { uint32_t elem_ctr, elem_actor, pred_ctr, pred_actor, count, flags; } am355_text_run;   /* actors: ranks, as in am355_patch_ir */
int am355_text_locate(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len,
                      uint64_t first, uint64_t n, const am355_text_run **runs, uint32_t *n_runs, uint64_t *length);
int am355_text_splice(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len,
                      uint64_t start, uint64_t deletions,
                      const uint8_t *utf8, const uint32_t *value_off, uint32_t n_values,   /* value i = utf8[value_off[i] .. value_off[i+1]) */
                      const uint8_t *author, size_t author_len, int64_t time, const uint8_t *message, uint32_t message_len,
                      const uint8_t **change, size_t *len);
int am355_text_splice_calls(const am355_ctx *ctx, uint64_t out[3]);   /* splices served | refused | device launches of the locate half */
int am355_text_locate_limits(uint32_t out[3]);                        /* the sizes at which the kernels switch path, for the tests */
/* The raw id of the actor with that rank (the ranks of am355_text_run and am355_patch_ir), without fetching the patch tables: *bytes is
 * owned by ctx and valid until the next call that changes the state. AM355_E_STATE: no replayed state; AM355_E_ARG: no such rank. */
int am355_actor_of_rank(const am355_ctx *ctx, uint32_t rank, const uint8_t **bytes, size_t *len);

/*
 * A plain LIST edited by POSITION (csrc/am355_list_locate.hip): what am355_text_locate / am355_text_splice are for a Text, for an object
 * made by makeList (type 2) -- doc.cards.deleteAt(3), doc.cards.insertAt(0, 7, 8, 9), doc.cards[2] = 'x' for a host without a frontend
 * document. The difference to a Text: an element of a list keeps EVERY conflicting value (frontend/apply_patch.js:156-213
 * updateListObject), and the pred of a deletion or an assignment names the op ids of all of them (context.js:576-586 getPred).
 * am355_list_locate resolves the elements [first, first + n) to runs: run = `count` elements whose elemIds are (elem_ctr + i, elem_actor).
 * A run of count > 1 has pred_num == 1 and element i's pred is ((*preds)[pred_first].ctr + i, .actor); a run of count == 1 has the
 * pred_num >= 1 preds (*preds)[pred_first .. pred_first + pred_num), in ascending op id (counter, then actor bytes) -- the order
 * am355_local_op wants. Runs are the deletions context.splice merges into `multiOp` (context.js:479-486: both elements have exactly one
 * pred, elemIds and preds of equal actors and consecutive counters); an element of several values is always a run of its own. Actors are
 * ranks, as in am355_patch_ir. (The reference's own exception is reproduced: `update` edits behind a `multi-insert` edit replace the
 * element's conflicts in its frontend, apply_patch.js:187-190, so the inserted value's id is not among the preds then; only a hand-made
 * `set` without pred onto an existing element makes such a history.) flags & AM355_RUN_COUNTER: the value the list SHOWS for some element of the run (the last one) is a Counter.
 * *runs / *preds are pinned memory owned by the context, valid until the next call on ctx; *length = list.length; n == 0 is legal and
 * returns the length. It reads only, as am355_text_locate does, with its contexts and errors (AM355_E_STATE, sharded
 * AM355_E_UNSUPPORTED, AM355_E_ARG "no such object: ..." / "not a list object" for anything but a plain list, first + n > length:
 * AM355_E_ARG, a `remove` record: AM355_E_UNSUPPORTED, records that contradict each other: AM355_E_DEVICE), and two of its own, both
 * AM355_E_UNSUPPORTED: an element whose first edit is an `update` (it was reported as `remove` first; the reference's frontend has no
 * elemId for it), and an element of more than 4096 values (the bound am355_apply_local_change has for the preds of one op).
 *
 * am355_list_splice: one context.splice(path, start, deletions, insertions) (context.js:441-502) on the list the context holds. It locates
 * [start - 1, start + deletions) in one query and builds the request of the frontend: one `del` per run of the deleted elements (multiOp =
 * count, pred = all preds), then insertListItems (context.js:370-405) behind element start - 1 (`_head` for start == 0): several values
 * that all carry the same datatype are ONE `set` with `values` (strings, booleans and null carry none and are one class; AM355_LV_INT,
 * _UINT, _FLOAT64, _COUNTER and _TIMESTAMP are each their own), otherwise one inserting `set` per value, each naming the element the op
 * before it made. Values are am355_local_value, as for am355_apply_local_change (AM355_LV_UTF8: a range of `strings`; AM355_LV_BYTES stays
 * refused there). seq, startOp, deps and the application are those of am355_text_splice. Decided before the state is touched (a document
 * context is at most turned into the state of its rebuilt changes): start > length - deletions: AM355_E_ARG with the reference's
 * RangeError text ("<deletions> deletions starting at index <start> are out of bounds for list of length <length>"); a deleted element
 * that shows a Counter: AM355_E_INVALID with its TypeError text ("Unsupported operation: deleting a counter from a list"; for a list the
 * reference really throws); deletions == 0 && n_values == 0: AM355_OK, *len = 0, nothing applied; the errors of am355_list_locate; queued
 * changes in the state: AM355_E_UNSUPPORTED. Inserting objects is not served: `child` ops are not in the flat request form.
 *
 * am355_list_set: list[index] = value (context.js:411-435 setListIndex). index >= length: a splice at `length` of index - length nulls
 * followed by the value (at most 2^20 nulls; more: AM355_E_UNSUPPORTED). Otherwise one `set`, insert: false, with the element's elemId and
 * pred = all its preds; onto an element that shows a Counter: AM355_E_INVALID with the reference's RangeError text ("Cannot overwrite a
 * Counter object; use .increment() or .decrement() to change its value."). THE CALL ALWAYS EMITS THE OP: the reference skips it when the
 * new value === the shown one and the element has at most one value; the engine holds no JS values, so a caller that wants that
 * economy compares before it calls.
 * am355_list_splice_calls: out[0] calls of am355_list_splice and am355_list_set served, out[1] refused (whatever the code), out[2] kernel
 * launches of the locate half of the three calls. am355_list_locate_limits: out[0] = elements one workgroup of the locate kernel takes,
 * out[1] = elements up to which the scan is one workgroup, out[2] = runs, and preds, written straight into pinned memory (the ones behind
 * go to device memory and down in one copy each).
 * Not built: am355_text_position for lists, increments of a counter inside a list (a map's: am355_map_update), a locate without the
 * rebuild of stale edit tables.
 */
typedef struct { uint32_t elem_ctr, elem_actor, count, flags, pred_first, pred_num; } am355_list_run;   /* flags: AM355_RUN_COUNTER; actors: ranks */
typedef struct { uint32_t actor, ctr; } am355_list_pred;                                               /* actor: a rank */
int am355_list_locate(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len, uint64_t first, uint64_t n,
                      const am355_list_run **runs, uint32_t *n_runs, const am355_list_pred **preds, uint32_t *n_preds, uint64_t *length);
int am355_list_splice(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len, uint64_t start, uint64_t deletions,
                      const am355_local_value *values, uint32_t n_values, const uint8_t *strings, uint32_t strings_len,
                      const uint8_t *author, size_t author_len, int64_t time, const uint8_t *message, uint32_t message_len,
                      const uint8_t **change, size_t *len);
int am355_list_set(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len, uint64_t index,
                   const am355_local_value *value, const uint8_t *strings, uint32_t strings_len,
                   const uint8_t *author, size_t author_len, int64_t time, const uint8_t *message, uint32_t message_len,
                   const uint8_t **change, size_t *len);
int am355_list_splice_calls(const am355_ctx *ctx, uint64_t out[3]);   /* served | refused | device launches of the locate half */
int am355_list_locate_limits(uint32_t out[3]);                        /* the sizes at which the kernels switch path, for the tests */

/*
 * A MAP edited by KEY (csrc/am355_map_locate.hip): doc.title = 'x', delete doc.draft, doc.votes.increment() for a host without a frontend
 * document, and "what does this key hold". A change request names the op ids of EVERY visible value of the key it touches (`pred`,
 * frontend/context.js:576-586 getPred); they stand in the map table, which is sorted by (object, key in UTF-16 code unit order, op id).
 * am355_map_locate resolves n keys of the map or table obj_ctr @ obj_actor (_root: obj_ctr == 0 && actor_len == 0) in one query: key i is
 * the UTF-8 bytes keys[key_off[i] .. key_off[i + 1]). (*hits)[i] = {first, num, flags, pad}: the key holds num visible values (0: the key
 * is absent), whose am355_ir_map records -- copied as they are: value, counter total, flags, op id with the actor as a RANK -- are
 * (*recs)[first .. first + num), in ascending op id (counter, then actor bytes): the order am355_local_op wants for preds. flags =
 * AM355_MAP_COUNTER / AM355_MAP_CHILD of the value the map SHOWS, which is the last record (the greatest op id,
 * frontend/apply_patch.js:57-79; AM355_MAP_COUNTER also for a counter nobody has incremented yet, whose record carries only the type of
 * its `set` and no total). A record's {id_ctr, id_actor} is the pred; for a child object it is also the child's objectId.
 * *n_recs = records gathered; a key asked for twice has its records twice (at most records of the object + n in all: beyond that
 * AM355_E_ARG). *hits / *recs are pinned memory owned by the context, valid until the next call on ctx. n == 0 and an object without
 * records launch nothing. On the device one wavefront searches per key, 64 pivots a round; before a record is copied the search has
 * verified itself (the keys on both sides of the run differ in the right direction, the ids inside it ascend, every key read lies in
 * the arena, no record is an AM355_MAP_EMPTY one): a miss is AM355_E_DEVICE, nothing is read or written out of range.
 * It reads only: the state, what serves the next am355_apply_changes, the host copies of the tables and the flags that describe them
 * stay as they were, and -- unlike the calls on a Text or a list -- edit tables that in-place merges left stale are NOT rebuilt: the
 * object and map tables are current behind every such merge. Served for map (type 0) and table (type 6) objects on the contexts
 * am355_object_text serves; AM355_E_STATE, sharded AM355_E_UNSUPPORTED, AM355_E_ARG "no such object: ..." as there; any other object:
 * AM355_E_ARG "not a map object".
 *
 * am355_map_update: ONE change on ONE map -- what Automerge.change(doc, d => { d.a = 1; delete d.b; d.n.increment(2) }) makes. All keys of
 * the call are located in one query; seq, startOp, deps and the application (small path, bulk path, patch, envelope) are those of
 * am355_text_splice. Keys are ranges of `strings`, as the UTF-8 values are; op i:
 *   AM355_MOP_SET     values[value] assigned (context.js:325-346, :289-309): one `set`, insert: false, pred = every id of the key. Value
 *                     classes as for am355_list_splice. An empty key: AM355_E_ARG "The key of a map entry must not be an empty string";
 *                     a key that shows a Counter: AM355_E_INVALID "Cannot overwrite a Counter object; use .increment() or .decrement()
 *                     to change its value.". THE OP IS ALWAYS EMITTED: the reference skips an assignment of the value the key already
 *                     shows without a conflict; the engine holds no JS values, a caller that wants that economy compares first.
 *   AM355_MOP_DELETE  (:351-362) a `del` with every id as pred; a key without a value emits no op. On a TABLE object (:531-540
 *                     deleteTableRow) this is the only kind served (one pred); anything else there: AM355_E_UNSUPPORTED.
 *   AM355_MOP_INC     (:546-573) an `inc` of `delta` with every id as pred; a key that is absent or shows no Counter: AM355_E_INVALID
 *                     "Only counter values can be incremented".
 * A context that holds NO state (a fresh or reset one -- and, as for am355_apply_local_change, one whose state a refused apply dropped)
 * is Backend.init(): _root without a key, seq 1, startOp 1, no deps; any other object is "no such object" there.
 * The ops are judged in their order and the first exception is the call's. A call that ends without an op (deletions of absent keys, no
 * ops) returns AM355_OK with *len = 0 and applies nothing. A key named twice in one call: AM355_E_ARG (the frontend would name the first
 * op as the second's pred: not built). Assigning objects is not served: `child` ops are not in the flat request form. All of this, and
 * the state errors of am355_list_splice (queued changes: AM355_E_UNSUPPORTED), is decided before the state is touched.
 * am355_map_calls: out[0] am355_map_update calls served, out[1] refused (whatever the code), out[2] kernel launches of the locate half of
 * both calls (the object lookup included; the library scan counts as one). am355_map_locate_limits: out[0] = records up to which an
 * object is searched by the last round alone (more: narrowing rounds first), out[1] = keys read from pinned memory (more: one copy up),
 * out[2] = hits, and records, written straight into pinned memory (the ones behind go to device memory and down in one copy each),
 * out[3] = G: the result arrays of the first gather have room for 2 n + G records (they are not sized for the bound above: one key asked
 * of a map of a million records would pin 40 MB); a call whose keys hold more -- many conflicting values per key -- learns the count in
 * its one wait, gathers a second time into arrays of that size and waits once more. A key of more than 256 bytes is compared where it
 * lies, not from LDS: a call that names one copies its keys up instead of reading them from pinned memory.
 * am355_set_map_locate_thread: on != 0: one thread per key and two binary searches instead of the wavefront -- the same answers; a
 * measurement switch (profiles/map_update_timings.txt), off by default.
 * Not built: assigning objects, a key named twice, am355_map_update across several objects in one change.
 */
enum { AM355_MOP_SET = 1, AM355_MOP_DELETE = 2, AM355_MOP_INC = 3 };       /* am355_map_op.kind */
typedef struct { uint32_t first, num, flags, pad; } am355_map_hit;         /* flags: AM355_MAP_COUNTER / AM355_MAP_CHILD of the shown value */
typedef struct {
  uint32_t kind;                   /* AM355_MOP_* */
  uint32_t key_off, key_len;       /* the key: a range of `strings` */
  uint32_t value;                  /* AM355_MOP_SET: index into `values` */
  int64_t delta;                   /* AM355_MOP_INC */
} am355_map_op;
int am355_map_locate(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len,
                     const uint8_t *keys, const uint32_t *key_off, uint32_t n,   /* key i = keys[key_off[i] .. key_off[i+1]) */
                     const am355_map_hit **hits, const am355_ir_map **recs, uint32_t *n_recs);
int am355_map_update(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len,
                     const am355_map_op *ops, uint32_t n_ops, const uint8_t *strings, uint32_t strings_len,
                     const am355_local_value *values, uint32_t n_values,
                     const uint8_t *author, size_t author_len, int64_t time, const uint8_t *message, uint32_t message_len,
                     const uint8_t **change, size_t *len);
int am355_map_calls(const am355_ctx *ctx, uint64_t out[3]);          /* updates served | refused | device launches of the locate half */
int am355_map_locate_limits(uint32_t out[4]);                        /* the sizes at which the kernels switch path, for the tests */
int am355_set_map_locate_thread(am355_ctx *ctx, int on);

/*
 * ElemIds of a Text resolved to POSITIONS (csrc/am355_position.hip): the inverse of am355_text_locate, and what keeps a caret, a
 * selection or a comment anchor alive while remote changes arrive -- the only stable name for a place in an RGA text is an elemId.
 * Query i is the element (ids[i].ctr, ids[i].actor) of the Text obj_ctr @ obj_actor; answer (*out)[i] is
 *   AM355_POS_VISIBLE  the element is in the Text: position = its index (text.getElemId(position) === elemId in the reference's frontend);
 *                      | AM355_POS_COUNTER when it is a Counter (the test of am355_text_locate's AM355_RUN_COUNTER);
 *   AM355_POS_DELETED  it was inserted into this Text and shows no value any more: position = the number of visible elements in front of
 *                      it in document order -- what the whole-document patch cannot say;
 *   AM355_POS_UNKNOWN  no applied change inserted such an element into this object (an unknown actor, a counter no row holds, a row that
 *                      is no insert, an element of another object): position = 0. No error: a cursor may name an element of a change
 *                      that has not arrived yet.
 * In both known cases the caret position directly behind the element is position + (status == AM355_POS_VISIBLE). The reference has no
 * cursor call; the number is pinned to it by a probe: a change of a fresh actor with startOp = maxOp + 1, deps = heads and the one op
 * {action: 'set', insert: true, elemId: X, pred: []} lands directly behind X, and the patch of Backend.applyChanges on a clone of the
 * state reports it at index = that caret position (tools/fixtures/make_text_positions.js).
 * Actors are RANKS, as in am355_text_run; 0xffffffff = an actor the state does not know. Ranks are renumbered when a new actor
 * arrives: a caller keeps actor bytes and asks for ranks per call (am355_rank_of_actor, the inverse of am355_actor_of_rank; no such
 * actor: AM355_E_ARG). *out is pinned memory owned by the context, valid until the next call on ctx; *length = the Text's length.
 * n == 0 is legal and returns the length.
 * Contexts and errors are those of am355_text_locate: AM355_E_STATE, AM355_E_UNSUPPORTED for a sharded context, AM355_E_ARG "no such
 * object: ..." / "not a Text object", AM355_E_UNSUPPORTED for a Text with a `remove` record, AM355_E_DEVICE for tables that contradict
 * each other (every row and every position is checked before it is used as an index). A DOCUMENT context is first turned into the state
 * of its rebuilt changes, exactly as am355_text_splice does: the search runs over the op rows and the stored list order, which a loaded
 * document does not have. Apart from that the call reads only: the state, what serves the next am355_apply_changes and the host
 * copies of the tables stay as they were (edit tables that in-place merges left stale are rebuilt once; the row -> position table of
 * the stored order is built when no in-place merge left it current, which is what the next in-place merge would have done itself).
 * am355_text_position_calls: out[0] = calls served, out[1] = kernel launches they made (the object lookup included). A Text without
 * records launches no heads pass; whether it has deleted elements only the device knows, so its queries are still resolved.
 * am355_text_position_limits: out[0] = queries (and records) one workgroup takes, out[1] = results written straight into pinned memory
 * (the ones behind go to device memory and down in one copy; up to that many queries are read from pinned memory too).
 */
enum { AM355_POS_UNKNOWN = 0u, AM355_POS_VISIBLE = 1u, AM355_POS_DELETED = 2u, AM355_POS_STATUS = 3u /* mask */, AM355_POS_COUNTER = 0x100u };
typedef struct { uint32_t ctr, actor; } am355_elem_id;         /* actor: a rank, as in am355_text_run; 0xffffffff = unknown actor */
typedef struct { uint32_t position, status; } am355_elem_pos;  /* status: AM355_POS_* | AM355_POS_COUNTER */
int am355_text_position(am355_ctx *ctx, uint64_t obj_ctr, const uint8_t *obj_actor, size_t actor_len,
                        const am355_elem_id *ids, uint32_t n, const am355_elem_pos **out, uint64_t *length);
int am355_rank_of_actor(const am355_ctx *ctx, const uint8_t *bytes, size_t len, uint32_t *rank);   /* inverse of am355_actor_of_rank; no such actor: AM355_E_ARG */
int am355_text_position_calls(const am355_ctx *ctx, uint64_t out[2]);   /* served | launches */
int am355_text_position_limits(uint32_t out[2]);                        /* queries per workgroup | results written to pinned memory */

/* ---- diagnostics: device primitives exposed for kernel-level tests ---- */
/* The device hash table of the queries above, driven by itself: a table over table_hashes (n_table x 32 bytes) is built and
 * queries (n_queries x 32 bytes) are probed, both on the device; out_idx[q] = index of the table hash equal to query q (the smallest,
 * when table_hashes holds a hash more than once), or 0xffffffff. The table has S = the smallest power of two >= max(64, 2 * n_table + 64)
 * slots; a hash starts at slot ((little-endian u64 of its first 8 bytes * 0x9e3779b97f4a7c15 mod 2^64) >> 32) & (S - 1) and takes the
 * first free slot from there on, wrapping behind the last one; a probe walks the same way to the first empty slot and compares all 32
 * bytes at every slot it passes. n_queries == 0 and n_table == 0 launch nothing. */
int am355_test_hash_probe(am355_ctx *ctx, const uint8_t *table_hashes, uint32_t n_table, const uint8_t *queries, uint32_t n_queries, uint32_t *out_idx);
int am355_test_sort(am355_ctx *ctx, uint64_t *keys, uint32_t *vals, uint32_t n, int key_bits);
int am355_test_scan(am355_ctx *ctx, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *total);
/* The primitives one by one (tests/test_primitives.py). Every buffer is an IMAGE: uploaded whole, handed to the primitive at the given
 * offset (scans: 0..3 words, so that the pointer is deliberately not 16-byte aligned; terminators: 0..7 bytes), downloaded whole -- the
 * caller sees the words around a range too. A range that would leave its image is refused with AM355_E_ARG, nothing is launched.
 *   scan_at / scan2: out_buf (out_a and out_b) NULL = in place (out_off == in_off); a NULL total is not asked for, else it holds the
 *     word's value before the call and after it.  scan_terminators: out has L + 1 entries.  max: *inout = *d_out before and after.
 *   sort_bits: first_table NULL, or the first digit's histogram computed by the caller ([digit * tiles + tile], tiles of 2048 pairs;
 *     AM355_E_ARG for sorts of more than 64 tiles); *result_buffer = 0 / 1, the buffer the sort named -- keys / vals come from there.
 *   remap: ranges = n_ranges x {first word, count, stride, guard (int32), guard_skip}; fill: x {first word, BYTES, value}; both with
 *     base_off (0..3 words) added to every first word.  copy: x {dst byte offset, src byte offset, bytes}, the source in pinned host
 *     memory (src_pinned) or in device memory.  AM355_E_ARG also when the range table's add() refuses a range; *n_added = ranges the
 *     table held at the launch.
 *   signal_words: host_words / *seq_word = the pinned words before and after the launch.
 *   carried_scan: out = exclusive prefix of v over the grid (carry_publish in one kernel, carry_prefix in the next); out_wg, wg_total
 *     [(n + 255) / 256] = exclusive prefix within each 256-thread workgroup and its sum (block_exclusive_scan_u32). */
int am355_test_scan_at(am355_ctx *ctx, uint32_t *in_buf, uint32_t in_words, uint32_t in_off, uint32_t *out_buf, uint32_t out_words, uint32_t out_off,
                       uint32_t n, uint32_t *total);
int am355_test_scan2(am355_ctx *ctx, uint32_t *in_a, uint32_t *in_b, uint32_t in_words, uint32_t in_off, uint32_t *out_a, uint32_t *out_b, uint32_t out_words,
                     uint32_t out_off, uint32_t n, uint32_t *total_a, uint32_t *total_b);
int am355_test_scan_terminators(am355_ctx *ctx, const uint8_t *bytes_buf, size_t bytes_len, uint32_t byte_off, uint32_t L, uint32_t *out_buf, uint32_t out_words,
                                uint32_t out_off, uint32_t *total);
int am355_test_max(am355_ctx *ctx, const uint32_t *v, uint32_t n, uint32_t *inout);
int am355_test_sort_bits(am355_ctx *ctx, uint64_t *keys, uint32_t *vals, uint32_t n, int begin_bit, int end_bit, const uint32_t *first_table, int *result_buffer);
int am355_test_chain_mark(am355_ctx *ctx, const uint32_t *next, uint32_t *mark, uint32_t mark_words, uint32_t n);
int am355_test_remap(am355_ctx *ctx, uint32_t *buf, uint32_t words, uint32_t base_off, const uint32_t *ranges, uint32_t n_ranges, const uint32_t *table, uint32_t n_old,
                     uint32_t *n_added);
int am355_test_fill(am355_ctx *ctx, uint32_t *buf, uint32_t words, uint32_t base_off, const uint32_t *ranges, uint32_t n_ranges, uint32_t *n_added);
int am355_test_copy(am355_ctx *ctx, uint8_t *dst, size_t dst_bytes, const uint8_t *src, size_t src_bytes, int src_pinned, const uint32_t *ranges, uint32_t n_ranges,
                    uint32_t *n_added);
int am355_test_signal_words(am355_ctx *ctx, const uint32_t *a, uint32_t n_a, const uint32_t *b, uint32_t n_b, uint32_t seq, uint32_t *host_words, uint32_t host_words_n,
                            uint32_t *seq_word);
int am355_test_carried_scan(am355_ctx *ctx, const uint32_t *v, uint32_t n, uint32_t *out, uint32_t *out_wg, uint32_t *wg_total);
/* The check pass of the calls on a Text (am355_text_locate, am355_text_splice, am355_text_position) over a hand-made record table:
 * `table` holds n_recs records, the sentinel among them, and the R >= 1 records from `begin` on are checked as those of one object
 * (begin + R + 1 <= n_recs: every record read lies in the table); n_values: values of the whole table. *flags: 1 = the records do not
 * continue each other or name values outside the table, 2 = a `remove` record. *length: in, what the length word holds before the
 * pass; out, what it holds behind it -- the object's length when flags == 0, else as it was. */
int am355_test_text_premises(am355_ctx *ctx, const am355_ir_edit *table, uint32_t n_recs, uint32_t begin, uint32_t R, uint32_t n_values, uint32_t *flags, uint32_t *length);
/* The check pass of the calls on a plain list (am355_list_locate, am355_list_splice, am355_list_set) over a hand-made record table: as
 * am355_test_text_premises, with the bit of the list calls beside the two premises -- 8 = an element whose first record carries
 * AM355_EDIT_UPDATE. */
int am355_test_list_premises(am355_ctx *ctx, const am355_ir_edit *table, uint32_t n_recs, uint32_t begin, uint32_t R, uint32_t n_values, uint32_t *flags, uint32_t *length);
/* decoded op rows of the last replay, copied to caller arrays of length n_ops (any pointer may be NULL) */
int am355_get_rows(am355_ctx *ctx, uint32_t *obj_actor, uint32_t *obj_ctr, uint32_t *key_actor, uint32_t *key_ctr, uint32_t *key_off,
                   uint32_t *key_len, uint32_t *action, uint32_t *val_tl, uint32_t *val_off, uint32_t *pred_num, uint32_t *id_ctr,
                   uint32_t *id_actor, uint8_t *insert, uint32_t *succ_cnt);

#ifdef __cplusplus
}
#endif
#endif
