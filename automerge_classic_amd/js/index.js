// mi355x-backend: drop-in replacement for automerge-classic's `backend` module whose bulk-replay path runs on an
// AMD MI355X through the N-API addon (am355_napi.node -> include/am355.h -> HIP kernels).
//
//   const Automerge = require('automerge')
//   Automerge.setDefaultBackend(require('mi355x-backend'))        // reference plug-in point: src/automerge.js:147-149
//
// Module surface = reference backend/index.js:1-8.  GPU-served calls (SURVEY.md "Scope decisions"):
//   loadChanges(init(), changes)  and  getPatch(state)             (backend/backend.js:116-129, new.js:1797-1879, 2060-2068)
//   applyChanges(state, changes) with its incremental patch        (backend/backend.js:27-31; SURVEY.md 8f-2) when `state` is empty
//                                                                  or was built by the engine
//   load / save / getAllChanges after load                         (SURVEY.md a21, 8f-1, 8f-3)
//   applyLocalChange(state, request) -> [state', patch, change]    (backend/backend.js:54-91) for the states applyChanges is served on:
//                                                                  the change is built on the device (local_change.js, am355_apply_local_change)
//   updateMap(state, objectId, ops, {actor, time, message}) / getMapValues(state, objectId, keys) / locateMap(state, objectId, keys)
//     ADDITIONS: a map edited by key -- d.key = v, delete d.key, d.key.increment(n) -- and what its keys hold (am355_map_update / _locate; see below)
//   positionsOfText(state, objectId, elemIds)   ADDITION: where elements of a Text stand now, deleted ones included (am355_text_position; see below)
//   spliceList(state, objectId, start, deletions, values, {actor, time, message}) / setListItem(state, objectId, index, value, options) /
//   locateList(state, objectId, first, n)   ADDITIONS: a plain list edited by position (am355_list_splice / _set / _locate; see below)
//   spliceText(state, objectId, start, deletions, strings, {actor, time, message}) / locateText(state, objectId, first, n)   ADDITIONS: a
//     Text edited by position, for hosts without a frontend document (am355_text_splice / am355_text_locate; see below)
//   getText(state, objectId) / getTextInfo(state, objectId)        ADDITIONS to the reference's surface: the string of a Text object read on
//                                                                  the device from the edit records (am355_object_text), no patch built
//   getChanges / getChangeByHash / getMissingDeps / getChangesAdded and the sync helpers over them: index lists from the engine's
//                                                                  hash-graph queries (am355_changes_since, am355_find_changes,
//                                                                  am355_missing_deps, am355_changes_added; new.js:1921-2028)
// Everything else (clone, requests the engine refuses) is delegated to the reference JS backend, onto
// which a GPU-built state is hydrated lazily -- by replaying the retained change buffers -- the first time such a
// call is made.  Inputs the engine rejects (AM355_E_INVALID: the reference would throw; AM355_E_UNSUPPORTED: legal
// but outside the GPU-served subset) are re-run on the JS path so the caller sees the reference's exact exception
// or result.  If the addon or the GPU is missing, requiring this module throws: there is no silent CPU mode
// (set MI355X_BACKEND_JS_ONLY=1 to run the pure pass-through plumbing configuration explicitly).
'use strict'
const path = require('path')

const JS_ONLY = process.env.MI355X_BACKEND_JS_ONLY === '1'
const HYDRATE_FROM_DOC = process.env.MI355X_HYDRATE === 'doc'
const MAP_MERGE = process.env.MI355X_MAP_MERGE === '1'   // am355_set_resident_map_merge for every context of this module
const NEW_OBJECTS = process.env.MI355X_NEW_OBJECTS !== '0'   // am355_set_resident_new_objects for every context of this module (MI355X_NEW_OBJECTS=0: off, for A/B)
const COUNTERS = process.env.MI355X_COUNTERS !== '0'   // am355_set_resident_counters for every context of this module (MI355X_COUNTERS=0: off, for A/B)
const LOCAL_SMALL = process.env.MI355X_LOCAL_SMALL !== '0'   // am355_set_local_small for every context of this module (MI355X_LOCAL_SMALL=0: off, for A/B)
const PATCH_VIA_JSON = process.env.MI355X_PATCH_VIA_JSON === '1'   // A/B: JSON text rendered by the engine + JSON.parse
const LOCAL_CHANGE = process.env.MI355X_LOCAL_CHANGE !== '0'   // applyLocalChange on the engine (MI355X_LOCAL_CHANGE=0: the reference path, for A/B)
const { materialize } = require('./materialize.js')
const { flatten, flattenValues } = require('./local_change.js')
let addon = null, ctx = null
// A few engine contexts, used least-recently-used first: a GPU-built state remembers which replay (generation) made it, and as
// long as that replay still sits in one of the contexts, Backend.save of the state is served from it instead of replaying the
// retained changes again (MI355X_CONTEXTS, default 4; every context owns its device buffers).
const MAX_CONTEXTS = Math.max(1, parseInt(process.env.MI355X_CONTEXTS || '4'))
const contexts = []
let tick = 0
let graphProbeMin = null   // _setGraphProbeMin: given to every context made later too (null: the library's default)
if (!JS_ONLY) {
  addon = require(path.join(__dirname, 'am355_napi.node'))
  ctx = addon.create(parseInt(process.env.MI355X_DEVICE || '0'))   // throws without an MI355X
  if (MAP_MERGE) addon.setResidentMapMerge(ctx, true)   // (as for every context acquireContext makes, see there)
  if (NEW_OBJECTS) addon.setResidentNewObjects(ctx, true)
  if (COUNTERS) addon.setResidentCounters(ctx, true)
  if (LOCAL_SMALL) addon.setLocalSmall(ctx, true)
  contexts.push({ ctx, generation: 0, used: 0 })
}

// The unmodified reference backend (the package a user already has installed)
let refBackend = null
function ref() {
  if (!refBackend) {
    const spec = process.env.AUTOMERGE_BACKEND_PATH || 'automerge/backend'
    refBackend = require(spec)
  }
  return refBackend
}

const AM355_E_ARG = -2, AM355_E_INVALID = -3, AM355_E_UNSUPPORTED = -4

// A state built on the GPU. `changes` are retained (by reference, like BackendDoc.changes new.js:1847) so that a
// JS BackendDoc can be hydrated later; `patch` is the whole-document patch computed by the engine.
class GpuState {
  constructor(changes, patch, heads, doc) {
    this.changes = changes   // retained change buffers (loadChanges), or null
    this.doc = doc || null   // retained document bytes (load), or null
    this.patch = patch
    this.heads = heads
    this.js = null           // hydrated reference backend handle
    this.generation = 0      // engine replay this state was built by (it may still sit in one of the contexts)
    this.applied = null      // input indexes of the applied changes, application order (loadChanges states)
    this.hashes = null       // 32 bytes per input change
    this.pending = 0
    this.byHash = null       // lazily: hex hash -> input index, applied changes only
    this.pendingIdx = null   // input indexes of the changes still queued (loadChanges / applyChanges states)
    this.inOrder = false     // every change applied in the order of `changes`, none queued: applied = 0 .. n - 1 (gpuApplyChanges)
    this.hashStore = null    // the growing buffer `hashes` is a view of, shared along a line of applyChanges calls
    this.calls = 1           // backend calls that built the state (1: one loadChanges / applyChanges onto an empty document)
    this.fromDocument = false // the lineage began with load(bytes): the reference's objectMeta came from the document, not from changes
    // How the reference would have come to this state, call by call: the document the lineage began with (or null) and the batch of
    // every loadChanges / applyChanges call since. hydrate() replays exactly these calls: what the reference's objectMeta.children
    // holds depends on where its calls ended (new.js:916-931), and a call the engine refused is re-run on a state that must be the
    // reference's own (ADVICE r3).
    this.baseDoc = null
    this.batches = null
  }
}
let generation = 0           // bumped by every GPU replay

// the context the next replay runs in (the least recently used one), stamped with a new generation
function acquireContext() {
  let e
  if (contexts.length < MAX_CONTEXTS && contexts.every(x => x.generation !== 0)) {
    e = { ctx: addon.create(parseInt(process.env.MI355X_DEVICE || '0')), generation: 0, used: 0 }
    // the first changes of a new collaborator are merged into the state the context holds (the reference appends the actor and touches
    // no stored op, new.js:1434-1451; the engine renumbers the actor ranks it stores) instead of replaying the whole log
    addon.setResidentNewActors(e.ctx, true)
    // key assignments are merged into the map records the context holds (the reference merges a batch into its stored op set and
    // touches only the blocks it visits, new.js:1052-1290) instead of every map value of the document being ordered again
    // (MI355X_MAP_MERGE=1: measured, the path gains nothing on one-change calls and is slower on 40-change calls, profiles/map_merge_timings.txt -- not the default here)
    if (MAP_MERGE) addon.setResidentMapMerge(e.ctx, true)
    // a change that makes objects (`doc.cards.push({...})`, `doc.notes = new Text(...)`: nearly every action on a structured document)
    // is merged into the state the context holds -- the new objects behind the stored ones, their elements at the end of the stored
    // order -- instead of every list being ranked and every table rebuilt (the reference inserts the ops into the blocks it visits,
    // new.js:1052-1290); measured faster than merge_run in every case timed, profiles/new_objects_apply_timings.txt: on unless MI355X_NEW_OBJECTS=0
    if (NEW_OBJECTS) addon.setResidentNewObjects(e.ctx, true)
    // a counter increment (`doc.votes.increment()`) rewrites the counter's stored map record in place instead of every list being ranked
    // and every table rebuilt (the reference adds the increment to the counter's succ list in the block it visits, new.js:1052-1290);
    // measured faster than merge_run in every case timed, profiles/counter_apply_timings.txt: on unless MI355X_COUNTERS=0
    if (COUNTERS) addon.setResidentCounters(e.ctx, true)
    // a keystroke (a change request of a few hundred rows at most) is built by one workgroup in one launch instead of by the bulk column
    // encoders (~115 stream commands); measured 0.18 against 0.54-0.62 ms for a typed character, 0.23-0.27 against 0.59-0.65 for 200, a paste beyond
    // the limits unchanged, profiles/local_small_timings.txt: on unless MI355X_LOCAL_SMALL=0
    if (LOCAL_SMALL) addon.setLocalSmall(e.ctx, true)
    if (graphProbeMin !== null) addon.setGraphProbeMin(e.ctx, graphProbeMin)
    contexts.push(e)
  } else {
    e = contexts.reduce((a, b) => (b.used < a.used ? b : a))
  }
  e.generation = ++generation
  e.used = ++tick
  ctx = e.ctx
  return e
}
// the context that still holds the replay of `gen`, if any
function contextOf(gen) {
  const e = contexts.find(x => x.generation === gen && gen !== 0)
  if (e) { e.used = ++tick; ctx = e.ctx }
  return e || null
}
const counters = { gpuLoadChanges: 0, gpuLoad: 0, gpuSave: 0, gpuHistory: 0, gpuApplyChanges: 0, gpuApplyLocalChange: 0, gpuChangesAdded: 0, localFallbacks: 0, saveReplays: 0, fallbackToJs: 0, hydrations: 0, gpuText: 0, textFallbacks: 0, gpuSplice: 0, spliceFallbacks: 0, gpuListSplice: 0, listSpliceFallbacks: 0, gpuPosition: 0, positionFallbacks: 0, gpuMap: 0, mapFallbacks: 0, gpuMapLocate: 0, mapLocateFallbacks: 0 }   // (diagnostics: which path served the calls)

function isFrozenCheck(backend) {
  // reference util.js:1-10
  if (backend.frozen) {
    throw new Error(
      'Attempting to use an outdated Automerge document that has already been updated. ' +
      'Please use the latest document state, or call Automerge.clone() if you really ' +
      'need to use this old document state.')
  }
}

function isEmptyRefState(backend) {
  const s = backend.state
  return s && !(s instanceof GpuState) && Array.isArray(s.changes) && s.changes.length === 0 &&
    (!s.queue || s.queue.length === 0) && !s.binaryDoc
}

// The JS (reference) handle equivalent to `backend`: a GPU-built state is hydrated once and the handle is cached on it.
// Read-only reference calls (clone, save, getAllChanges, getChanges, getChangesAdded, getChangeByHash, getMissingDeps,
// generateSyncMessage) use it WITHOUT freezing anything, as the reference never freezes on those (backend.js:12-14, 93-98,
// 139-196): `Automerge.load(bytes)` -> `getAllChanges(doc)` -> `Automerge.change(doc)` must keep working.
function hydrate(backend) {
  isFrozenCheck(backend)
  if (!(backend.state instanceof GpuState)) return backend
  const g = backend.state
  if (!g.js) {
    counters.hydrations++
    if (g.doc) { g.js = ref().load(g.doc); if (g.graphKnown && !g.js.state.haveHashGraph) g.js.state.computeHashGraph() }
    else if (HYDRATE_FROM_DOC && !JS_ONLY) {
      // hydrate the JS BackendDoc from the engine's save() bytes: Backend.load of a document is several times cheaper in JS than
      // replaying every change (opt-in: MI355X_HYDRATE=doc; the default replays the retained changes, exact by construction)
      let bytes = null
      try {
        if (!contextOf(g.generation)) replayForReading(g)
        bytes = addon.save(ctx, 0)
      } catch (e) {
        if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED) throw e
      }
      g.js = bytes ? ref().load(bytes) : ref().loadChanges(ref().init(), g.changes)
    } else if (g.batches) {
      let handle = g.baseDoc ? ref().load(g.baseDoc) : ref().init()
      for (const batch of g.batches) {
        if (batch === GRAPH_QUERY) { if (!handle.state.haveHashGraph) handle.state.computeHashGraph() } else handle = ref().loadChanges(handle, batch)
      }
      g.js = handle
    } else g.js = ref().loadChanges(ref().init(), g.changes)
  }
  return g.js
}

// Mutating reference calls (applyChanges, applyLocalChange, loadChanges, receiveSyncMessage) TAKE the JS handle: the
// reference freezes the handle it is given and returns a new one (backend.js:9-31, util.js:1-10), so the wrapper handle is
// frozen with it.
function toJs(backend) {
  const handle = hydrate(backend)
  if (backend.state instanceof GpuState) {
    backend.state.js = null
    backend.frozen = true
  }
  return handle
}

// the patch object of the last replay: built from the record tables the device wrote (materialize.js) -- real JS values, no
// JSON text in between
function gpuPatch() {
  return PATCH_VIA_JSON ? JSON.parse(addon.patchJSON(ctx)) : materialize(addon.fetchIR(ctx, true))
}

function gpuReplay(changes) {
  acquireContext()
  addon.loadChanges(ctx, changes)
  addon.replay(ctx)
  return gpuPatch()
}

// The retained changes of `g` replayed into a fresh context, in one go. When that is not how the state came to be -- several calls
// built it, or its lineage began with a loaded document -- the engine is told (am355_forget_call_history: how many of the leading changes
// are the document's): the few patches of later applyChanges calls that depend on where the reference's calls ended, or on whether it
// had rebuilt the document's hash graph by then, are refused instead of guessed
function replayRetained(g) {
  gpuReplay(g.changes)
  g.generation = generation
  g.fromChanges = true
  if (g.calls > 1 || g.fromDocument || g.doc) addon.forgetCallHistory(ctx, g.doc ? g.changes.length : (g.docChanges || 0))
  if (g.fromDocument || g.doc) addon.hashGraphKnown(ctx, g.graphKnown ? 1 : 0)
}

// A lineage that began with a loaded document can hold queued changes whose dependencies ARE in the document: the call in which the
// reference rebuilt its hash graph forgot the hashes of what it had applied before (new.js:1837-1840), and what depended on those waits
// for the next call. A replay of all retained changes would apply them too early: such a state is replayed from its APPLIED changes
// only, and the next applyChanges hands the queue over behind its batch (the reference's queue is batch ++ queue, new.js:1822).
const heldBack = g => !!(g.fromDocument && g.pendingIdx && g.pendingIdx.length > 0)
const appliedOnly = g => Array.from(g.applied, i => g.changes[i])
function replayForReading(g) {   // whole-document patch / save of a state whose context has moved on
  if (heldBack(g)) return gpuReplay(appliedOnly(g))   // (the context then holds nobody's list: g.generation stays as it is)
  const patch = gpuReplay(g.changes)
  g.generation = generation
  return patch
}

function init() {
  return ref().init()
}

function loadChanges(backend, changes) {
  isFrozenCheck(backend)
  if (!JS_ONLY && isEmptyRefState(backend) && Array.isArray(changes) && changes.length > 0) {
    try {
      const patch = gpuReplay(changes)
      counters.gpuLoadChanges++
      backend.frozen = true
      const state = new GpuState(changes.slice(), patch, patch.deps)
      state.batches = [state.changes]
      state.generation = generation
      state.applied = addon.appliedOrder(ctx)
      state.pendingIdx = addon.pendingOrder(ctx)
      state.hashes = addon.hashes(ctx)
      state.pending = patch.pendingChanges
      return { state, heads: patch.deps }
    } catch (e) {
      if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED && !(e instanceof TypeError)) throw e
      counters.fallbackToJs++
      // fall through: the reference path raises the exact exception (or serves the unsupported case)
    }
  }
  return ref().loadChanges(toJs(backend), changes)
}

function getPatch(backend) {
  isFrozenCheck(backend)
  if (backend.state instanceof GpuState) {
    const g = backend.state
    if (!g.patch) {
      // a state made by applyChanges: the whole-document patch is built when somebody asks for it (the engine context that
      // replayed the state still holds its record tables, else the retained changes are replayed)
      if (contextOf(g.generation)) g.patch = gpuPatch()
      else g.patch = replayForReading(g)
    }
    return g.patch
  }
  return ref().getPatch(backend)
}

function getHeads(backend) {
  return backend.heads   // reference backend.js:135-137
}

function load(data) {
  // Backend.load(bytes) (backend.js:104-107, new.js:1695-1750): header / checksum / inflate on the host, op-column decode and
  // whole-document patch on the GPU
  if (!JS_ONLY && data instanceof Uint8Array) {
    try {
      acquireContext()
      addon.backendLoad(ctx, data)
      const patch = gpuPatch()
      counters.gpuLoad++
      const state = new GpuState(null, patch, patch.deps, data)
      state.generation = generation
      return { state, heads: patch.deps }
    } catch (e) {
      if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED && !(e instanceof TypeError)) throw e
      counters.fallbackToJs++
    }
  }
  return ref().load(data)
}

// Backend.save(state) (backend.js:93-95, new.js:2033-2055). A GPU-built state is saved by the engine: canonical row order and
// column encoding on the GPU, document assembly / DEFLATE / checksum on the host. If the engine context has moved on to
// another document since, the retained changes are replayed first (still far cheaper than the JS path).
function save(backend) {
  isFrozenCheck(backend)
  const g = backend.state
  if (!JS_ONLY && g instanceof GpuState) {
    if (g.doc) return g.doc   // unchanged loaded document: the bytes it was loaded from (new.js:2034)
    try {
      if (!contextOf(g.generation)) { counters.saveReplays++; replayForReading(g) }
      const bytes = addon.save(ctx, 0)
      counters.gpuSave++
      return bytes
    } catch (e) {
      if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED) throw e
    }
  }
  return ref().save(hydrate(backend))
}

// History queries on a state built by loadChanges: the engine knows which changes were applied and in what order, and the
// change buffers are retained, so these need no JS BackendDoc. (Loaded documents and anything involving queued changes
// go to the reference path.)
function gpuHistory(backend, withQueue) {
  const g = backend.state
  if (JS_ONLY || !(g instanceof GpuState) || g.js) return null
  if (g.doc && !g.changes && !g.noHistory) loadedHistory(g)
  if (heldBack(g)) return null   // (its context list is not g.changes: the reference path, on the handle hydrate() makes call by call)
  return g.changes && g.applied && (g.pending === 0 || withQueue) ? g : null
}
// A BackendDoc made by load() rebuilds its hash graph IN PLACE when it is asked for changes, a change by hash, missing dependencies or
// a clone (new.js:1774, 1922, 1980, 2000, 2015) -- and schedules later applyChanges calls differently from then on (new.js:1826-1840).
// The wrapper serves those queries without a BackendDoc: it remembers that the reference would have the graph (am355_hash_graph_known).
const GRAPH_QUERY = Object.freeze([])   // (in GpuState.batches: here the reference rebuilt the hash graph because it was asked, see hydrate())
function noteGraphQuery(backend) {
  const g = backend && backend.state
  if (g instanceof GpuState && (g.doc || g.fromDocument) && !g.graphKnown) {
    g.graphKnown = true
    if (g.batches) g.batches = g.batches.concat([GRAPH_QUERY])
    if (g.js && !g.js.state.haveHashGraph) g.js.state.computeHashGraph()
  }
}
// History of a LOADED document (new.js:1887-1912 computeHashGraph, columnar.js:876-981): the engine rebuilds the binary changes
// and their hashes from the rows it decoded (am355_doc_changes) -- once, on the first history query, as the reference defers it.
// Documents it does not rebuild (or whose heads do not match) go to the reference path, which serves them or throws its error.
function loadedHistory(g) {
  try {
    if (!contextOf(g.generation)) {
      acquireContext()
      addon.loadDocument(ctx, g.doc)
      addon.replay(ctx)
      g.generation = generation
    }
    const h = addon.docChanges(ctx, 1)
    g.changes = h.changes
    g.hashes = h.hashes
    g.applied = Uint32Array.from(h.changes, (_, i) => i)
    g.pendingIdx = new Uint32Array(0)
    g.pending = 0
    counters.gpuHistory++
  } catch (e) {
    if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED) throw e
    g.noHistory = true
    counters.fallbackToJs++
  }
}
// The engine's own hash-graph queries serve a state while its context is live -- the replay that made the state still sits in it, so
// the context's list of changes is g.changes index for index -- and holds changes: not a state whose queue is kept out of the
// context (heldBack), not a loaded document that sits there as a document. Otherwise the JS restatements below run (hashIndex,
// graphOf), which build their indexes per state.
function engineGraph(g) {
  if (JS_ONLY || heldBack(g) || (g.doc && !g.fromChanges)) return false
  return !!contextOf(g.generation)
}
const HEX64 = /^[0-9a-f]{64}$/
// hashes given as hex strings, packed for the addon; null when one of them is not the hex of 32 bytes (the JS path then answers as
// the reference does for such a string)
function packHashes(list) {
  const out = Buffer.alloc(32 * list.length)
  for (let k = 0; k < list.length; k++) {
    if (typeof list[k] !== 'string' || !HEX64.test(list[k])) return null
    out.write(list[k], 32 * k, 'hex')
  }
  return new Uint8Array(out.buffer, out.byteOffset, out.length)
}
// index of the applied change with that hash, or undefined
function indexOfHash(g, hash) {
  if (engineGraph(g)) {
    const one = packHashes([hash])
    if (one) { const i = addon.findChanges(ctx, one)[0]; return i === 0xffffffff ? undefined : i }
  }
  return hashIndex(g).get(hash)
}
function hashIndex(g) {
  if (!g.byHash) {
    g.byHash = new Map()
    for (const i of g.applied) g.byHash.set(Buffer.from(g.hashes.buffer, g.hashes.byteOffset + 32 * i, 32).toString('hex'), i)
  }
  return g.byHash
}
function getAllChanges(backend) {   // new.js:1924-1927: BackendDoc.changes in application order (queued changes are not among them)
  isFrozenCheck(backend)
  noteGraphQuery(backend)
  const g = gpuHistory(backend, true)
  if (g) return Array.from(g.applied, i => g.changes[i])
  return ref().getAllChanges(hydrate(backend))
}
function getChanges(backend, haveDeps) {   // backend.js:152-157, new.js:1921-1976
  isFrozenCheck(backend)
  noteGraphQuery(backend)
  if (!Array.isArray(haveDeps)) throw new TypeError('Pass an array of hashes to Backend.getChanges()')
  const g = gpuHistory(backend, true)
  if (g) return changesSince(g, haveDeps).map(i => g.changes[i])
  return ref().getChanges(hydrate(backend), haveDeps)
}
function getChangeByHash(backend, hash) {   // new.js:1999-2002 (applied changes only: queued ones have no index)
  isFrozenCheck(backend)
  noteGraphQuery(backend)
  const g = gpuHistory(backend, true)
  if (g) { const i = indexOfHash(g, hash); return i === undefined ? undefined : g.changes[i] }
  return ref().getChangeByHash(hydrate(backend), hash)
}
function getMissingDeps(backend, heads = []) {   // new.js:2014-2028
  isFrozenCheck(backend)
  noteGraphQuery(backend)
  const g = gpuHistory(backend, true)
  if (g && g.pendingIdx) return missingDeps(g, heads)
  return ref().getMissingDeps(hydrate(backend), heads)
}

// Backend.applyChanges(backend, changes) -> [backend', patch] (backend.js:27-31, new.js:1797-1879) on the engine: the state is empty
// (applyChanges(init(), changes): everything arrives in one batch) or was built by the engine, whose context then replays the
// earlier changes and the batch together and derives the incremental patch on the device (am355_apply_changes). What the engine
// refuses (an assignment to a list element, an edit inside an object the document no longer reaches ...) or rejects is served by
// the reference path, which returns the reference's patch or throws its exception.
// 0 .. n - 1 as a view of one shared array (application order of a state whose changes all applied in the order they were given)
const EMPTY_U32 = new Uint32Array(0)
let IDENTITY = new Uint32Array(0)
function identity(n) {
  if (n > IDENTITY.length) {
    IDENTITY = new Uint32Array(Math.max(2 * n, 1024))
    for (let i = 0; i < IDENTITY.length; i++) IDENTITY[i] = i
  }
  return IDENTITY.subarray(0, n)
}
// The hashes of the n changes of `state` (all applied in input order). States along one line of calls share a growing store: the
// state at its tip appends the batch's hashes (fetched alone), a state that is not the tip -- a fork -- starts a store of its own.
function hashesExtended(g, state, n) {
  const have = g && g.inOrder && g.hashes && g.hashStore && g.hashStore.used === g.hashes.length && g.hashes.length <= 32 * n ? g.hashes.length / 32 : -1
  let store = have >= 0 ? g.hashStore : null
  if (store && 32 * n <= store.buf.length) {
    if (n > have) store.buf.set(addon.hashes(ctx, have), 32 * have)
  } else {
    const all = addon.hashes(ctx)
    store = { buf: new Uint8Array(Math.max(64 * n, 4096)), used: 0 }
    store.buf.set(all, 0)
  }
  store.used = 32 * n
  state.hashStore = store
  return store.buf.subarray(0, 32 * n)
}

// (AM355_JS_PROFILE=1: where a served applyChanges call spends its time -- before the engine call, in it, fetch + materialise, the new state)
const PROFILE = !!process.env.AM355_JS_PROFILE
const now = () => Number(process.hrtime.bigint()) / 1e6
const profile = { calls: 0, before_ms: 0, engine_ms: 0, patch_ms: 0, state_ms: 0 }
// The context that holds the state of `backend` (replayed into one if none does), ready for a call that goes onto it; null: the
// state's history is not to be had from the engine (the reference path serves the call). handed: queued changes that are not in the
// context (see heldBack), to be given behind the batch.
function contextForApply(backend) {
  const g = backend.state instanceof GpuState ? backend.state : null
  if (g && g.doc && !g.changes) {
    loadedHistory(g)   // a loaded document: its changes, rebuilt by the engine (am355_doc_changes)
    if (!g.changes) return null
  }
  if (g && !g.changes) return null
  let entry, handed = null   // handed: queued changes that are not in the context (see heldBack), given behind the batch
  if (g && g.doc) {
    // an unchanged loaded document: the engine applies the batch onto the DOCUMENT in its context (am355_apply_changes rebuilds the
    // hash graph as the reference's first applyChanges after load does, and knows that objectMeta came from the document's rows)
    if (g.fromChanges || !(entry = contextOf(g.generation))) {
      entry = acquireContext()
      addon.loadDocument(ctx, g.doc)
      addon.replay(ctx)
      g.generation = generation
      g.fromChanges = false
    }
  } else if (g) {
    if (!(entry = contextOf(g.generation))) {
      if (heldBack(g)) {
        gpuReplay(appliedOnly(g))
        addon.forgetCallHistory(ctx, g.docChanges || 0)
        addon.hashGraphKnown(ctx, g.graphKnown ? 1 : 0)
        handed = Array.from(g.pendingIdx, i => g.changes[i])
      } else replayRetained(g)
      entry = contextOf(generation)
    }
    if (!g.applied || !g.pendingIdx) { g.applied = addon.appliedOrder(ctx); g.pendingIdx = addon.pendingOrder(ctx) }
  } else {
    entry = acquireContext()
    addon.reset(ctx)
  }
  const docLineage = !!(g && (g.doc || g.fromDocument))
  if (docLineage && g.graphKnown) addon.hashGraphKnown(ctx, 1)
  return { g, entry, handed, docLineage }
}

function gpuApplyChanges(backend, changes) {
  const tpIn = PROFILE ? now() : 0
  const at = contextForApply(backend)
  if (!at) return null
  const { entry, handed } = at
  const tp0 = PROFILE ? now() : 0
  try {
    addon.applyChanges(ctx, handed ? changes.concat(handed) : changes)
  } catch (e) {
    entry.generation = 0   // (whatever the context holds now is nobody's state)
    throw e
  }
  const tp1 = PROFILE ? now() : 0
  const patch = materialize(addon.fetchApplyIR(ctx, true))
  const tp2 = PROFILE ? now() : 0
  const result = stateAfterApply(at, changes, patch, false)
  counters.gpuApplyChanges++
  if (PROFILE) { const tp3 = now(); profile.calls++; profile.before_ms += tp0 - tpIn; profile.engine_ms += tp1 - tp0; profile.patch_ms += tp2 - tp1; profile.state_ms += tp3 - tp2 }
  return result
}

// The new state behind a call the engine served on the context of contextForApply: `changes` is the batch (a local change: the one
// binary change the engine made). graphFirst: the reference rebuilt the document's hash graph BEFORE it applied the batch
// (applyLocalChange looking for the author's last hash, backend.js:38-39).
function stateAfterApply({ g, entry, handed, docLineage }, changes, patch, graphFirst) {
  // the engine's list of changes: those applied so far in application order, the batch, those that were queued
  const list = !g ? changes.slice() : g.inOrder ? g.changes.concat(changes)
    : Array.from(g.applied, i => g.changes[i]).concat(changes, Array.from(g.pendingIdx, i => g.changes[i]))
  const state = new GpuState(list, null, patch.deps)
  entry.generation = ++generation
  state.generation = generation
  // The usual call -- everything applied in the order it was given, nothing queued -- needs none of the per-change tables copied out of
  // the context: the application order is 0 .. n - 1, the queue is empty, and the hashes of the earlier changes are the previous
  // state's (a call on a 4 k-change document spent 0.27 ms on these copies, more than the engine on the batch).
  state.inOrder = !handed && addon.appliedInInputOrder(ctx)
  if (state.inOrder) {
    state.applied = identity(list.length)
    state.pendingIdx = EMPTY_U32
    state.hashes = hashesExtended(g, state, list.length)
  } else {
    state.applied = addon.appliedOrder(ctx)
    state.pendingIdx = addon.pendingOrder(ctx)
    state.hashes = addon.hashes(ctx)
  }
  state.pending = patch.pendingChanges
  state.calls = g ? g.calls + 1 : 1
  state.fromDocument = !!(g && (g.fromDocument || g.doc))
  state.graphKnown = docLineage ? addon.hashGraphKnown(ctx, -1) : undefined   // (has this call made the reference rebuild the document's hash graph?)
  state.docChanges = g ? (g.doc ? g.changes.length : (g.docChanges || 0)) : 0   // the leading changes that are a loaded document's
  state.baseDoc = g ? (g.baseDoc || g.doc || null) : null
  state.batches = (g && g.batches ? g.batches : (g && g.doc && g.graphKnown ? [GRAPH_QUERY] : [])).concat(graphFirst ? [GRAPH_QUERY] : [], [changes.slice()])
  return [{ state, heads: state.heads }, patch]
}

// Backend.applyLocalChange(backend, request) -> [backend', patch, binaryChange] (backend.js:54-91) on the engine, for the states
// applyChanges is served on: the request is flattened (local_change.js), the engine builds the binary change on the device, applies it
// as a one-change batch onto the state its context holds and returns the change; the patch carries `actor` and `seq` and its deps
// leave out the change's own hash, the state's heads do not (backend.js:88-90). A lineage that began with a loaded document: the
// engine notices when the reference would rebuild the document's hash graph to find the author's last hash (am355.h), and the new
// state remembers it as a graph query in front of the batch. null: not served (the reference path runs the request).
function gpuApplyLocalChange(backend, request) {
  const flat = flatten(request)
  const at = contextForApply(backend)
  if (!at || at.handed) return null
  const knownBefore = at.docLineage ? !!addon.hashGraphKnown(ctx, -1) : true
  let binaryChange
  try {
    binaryChange = addon.applyLocalChange(ctx, flat)
  } catch (e) {
    at.entry.generation = 0   // (whatever the context holds now is taken to be nobody's state: the reference path goes on from here)
    throw e
  }
  const ir = addon.fetchApplyIR(ctx, true)
  const patch = materialize(ir)
  const graphFirst = at.docLineage && !knownBefore && !!addon.hashGraphKnown(ctx, -1)
  const result = stateAfterApply(at, [binaryChange], patch, graphFirst)
  // the state's heads are the document's, the new change's hash among them (backend.js:90 returns state.heads, not patch.deps)
  const own = hexOfHash(result[0].state, result[0].state.hashes.length / 32 - 1)
  const heads = patch.deps.concat([own]).sort()
  result[0].state.heads = heads
  result[0].heads = heads
  counters.gpuApplyLocalChange++
  return [result[0], patch, binaryChange]
}
function applyLocalChange(backend, request) {
  isFrozenCheck(backend)
  const served = !JS_ONLY && LOCAL_CHANGE && ((backend.state instanceof GpuState && !backend.state.js) || isEmptyRefState(backend))
  if (served) {
    try {
      const result = gpuApplyLocalChange(backend, request)
      if (result) { backend.frozen = true; return result }
      counters.localFallbacks++
    } catch (e) {
      if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED && !(e instanceof TypeError)) throw e
      counters.localFallbacks++
    }
  }
  // (the reference freezes the handle it is given only once the request is through, backend.js:85: a request it throws on leaves the
  // wrapper's handle usable as well)
  const handle = hydrate(backend)
  const result = ref().applyLocalChange(handle, request)
  if (backend.state instanceof GpuState) { backend.state.js = null; backend.frozen = true }
  return result
}

function applyChanges(backend, changes) {
  isFrozenCheck(backend)
  const served = !JS_ONLY && Array.isArray(changes) && changes.length > 0 && changes.every(c => c instanceof Uint8Array) &&
    ((backend.state instanceof GpuState && !backend.state.js) || isEmptyRefState(backend))
  if (served) {
    try {
      const result = gpuApplyChanges(backend, changes)
      if (result) { backend.frozen = true; return result }
    } catch (e) {
      if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED && !(e instanceof TypeError)) throw e
      counters.fallbackToJs++
    }
  }
  return ref().applyChanges(toJs(backend), changes)
}

function free(backend) {
  if (backend.state instanceof GpuState) { backend.state = null; backend.frozen = true } else ref().free(backend)
}

// ---------------------------------------------------------------------------------------------------------------------------
// Sync protocol (SURVEY.md 8f-4; reference backend/sync.js).  A message that carries changes is applied by applyChanges above --
// the bulk receive runs on the engine --, and what generateSyncMessage computes over the hash graph of an engine-built state is
// served from the engine too: the dependency graph by index (resolved on the device while the changes were hashed), the Bloom
// filter over the hashes of the changes since the last sync built on the device, filters received from the peer probed there.
// The protocol logic itself (what to send when, the bookkeeping about the peer, the wire encoding) is the reference's own sync.js,
// bound to this module by boundSync() below.
// ---------------------------------------------------------------------------------------------------------------------------
function hexOfHash(g, i) { return Buffer.from(g.hashes.buffer, g.hashes.byteOffset + 32 * i, 32).toString('hex') }

// the engine context that holds the replay of `g` (replayed again from the retained changes when it has moved on)
function ensureContext(g) {
  // (a loaded document sits in its context as a document: the hash graph needs the replay of its rebuilt changes)
  if ((g.doc && !g.fromChanges) || !contextOf(g.generation)) { replayRetained(g); contextOf(generation) }
}

// hash graph of an engine-built state, by index into g.changes: dependencies as resolved on the device, dependents in the order the
// reference pushes them (new.js:1853-1856: in application order, every change onto the lists of its dependencies)
// the dependencies alone (what getChangesToSend walks among the changes it may send): no per-state map of dependents
function depsOf(g) {
  if (g.graph) return g.graph
  if (!g.deps) { ensureContext(g); g.deps = addon.depGraph(ctx) }
  return g.deps
}
function graphOf(g) {
  if (!g.graph) {
    const { depFirst, depIndex } = depsOf(g)
    const applied = new Uint8Array(g.changes.length)
    for (const i of g.applied) applied[i] = 1
    const dependents = new Map()
    for (const i of g.applied) {
      if (!dependents.has(i)) dependents.set(i, [])
      for (let k = depFirst[i]; k < depFirst[i + 1]; k++) {
        const d = depIndex[k]
        if (!dependents.has(d)) dependents.set(d, [])
        dependents.get(d).push(i)
      }
    }
    g.graph = { depFirst, depIndex, applied, dependents }
  }
  return g.graph
}

// BackendDoc.getChanges(haveDeps) (new.js:1921-1976) as a list of indexes, in the order the reference returns the changes
function changesSince(g, haveDeps) {
  if (haveDeps.length === 0) return Array.from(g.applied)
  const packed = engineGraph(g) ? packHashes(haveDeps) : null
  if (packed) {
    try {
      return Array.from(addon.changesSince(ctx, packed))
    } catch (e) {
      if (e.am355Code === AM355_E_INVALID && e.message.startsWith('hash not found: ')) throw new RangeError(e.message)   // new.js:1934
      if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED) throw e
    }
  }
  const idx = hashIndex(g), { depFirst, depIndex, dependents } = graphOf(g)
  let stack = [], seen = new Set(), toReturn = []
  for (const hash of haveDeps) {
    const i = idx.get(hash)
    if (i === undefined) throw new RangeError(`hash not found: ${hash}`)
    seen.add(i)
    stack.push(...dependents.get(i))
  }
  const depsSeen = i => { for (let k = depFirst[i]; k < depFirst[i + 1]; k++) if (!seen.has(depIndex[k])) return false; return true }
  while (stack.length > 0) {
    const i = stack.pop()
    seen.add(i)
    toReturn.push(i)
    if (!depsSeen(i)) break
    stack.push(...dependents.get(i))
  }
  const heads = g.heads.map(h => idx.get(h))
  if (stack.length === 0 && heads.every(h => seen.has(h))) return toReturn
  stack = haveDeps.map(h => idx.get(h))
  seen = new Set()
  while (stack.length > 0) {
    const i = stack.pop()
    if (!seen.has(i)) {
      for (let k = depFirst[i]; k < depFirst[i + 1]; k++) stack.push(depIndex[k])
      seen.add(i)
    }
  }
  return Array.from(g.applied).filter(i => !seen.has(i))
}

let refColumnar = null
function columnar() {
  if (!refColumnar) refColumnar = require(path.join(process.env.AUTOMERGE_BACKEND_PATH || 'automerge/backend', 'columnar'))
  return refColumnar
}

// BackendDoc.getMissingDeps(heads) (new.js:2014-2028) with a queue: the dependencies of the queued changes and the given heads that
// are neither applied nor queued
function missingDeps(g, heads) {
  const packed = engineGraph(g) && Array.isArray(heads) ? packHashes(heads) : null
  if (packed) {
    try {
      const raw = addon.missingDeps(ctx, packed), out = []
      for (let k = 0; k < raw.length; k += 32) out.push(Buffer.from(raw.buffer, raw.byteOffset + k, 32).toString('hex'))
      return out
    } catch (e) {
      if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED) throw e
    }
  }
  const idx = hashIndex(g), allDeps = new Set(heads), inQueue = new Set()
  for (const i of g.pendingIdx) {
    inQueue.add(hexOfHash(g, i))
    for (const dep of columnar().decodeChangeMeta(g.changes[i], false).deps) allDeps.add(dep)
  }
  const missing = []
  for (const hash of allDeps) if (!idx.has(hash) && !inQueue.has(hash)) missing.push(hash)
  return missing.sort()
}

function leb32(out, v) { do { let b = v & 0x7f; v >>>= 7; if (v) b |= 0x80; out.push(b) } while (v) }
function readLeb32(bytes, pos) {
  let v = 0, shift = 0
  for (;;) {
    if (pos.i >= bytes.length) throw new RangeError('buffer ended with incomplete number')
    const b = bytes[pos.i++]
    v += (b & 0x7f) * Math.pow(2, shift)
    shift += 7
    if (!(b & 0x80)) break
    if (shift > 35) throw new RangeError('number out of range')
  }
  if (v > 0xffffffff) throw new RangeError('number out of range')
  return v
}

// makeBloomFilter (sync.js:234-238): the filter over the changes applied since `lastSync`, its bits set on the device
function makeBloomFilterGpu(g, lastSync) {
  const list = changesSince(g, lastSync)
  if (list.length === 0) return { lastSync, bloom: new Uint8Array(0) }
  ensureContext(g)
  const bits = addon.bloomBuild(ctx, Uint32Array.from(list))
  const head = []
  leb32(head, list.length); leb32(head, 10); leb32(head, 7)   // numEntries, BITS_PER_ENTRY, NUM_PROBES (sync.js:31, 66-74)
  const bloom = new Uint8Array(head.length + bits.length)
  bloom.set(head)
  bloom.set(bits, head.length)
  return { lastSync, bloom }
}

// getChangesToSend (sync.js:246-306) over indexes; the peer's filters are probed on the device
function changesToSendGpu(backend, g, have, need) {
  if (have.length === 0) return need.map(hash => getChangeByHash(backend, hash)).filter(change => change !== undefined)
  const lastSyncHashes = {}, filters = []
  for (const h of have) {
    for (const hash of h.lastSync) lastSyncHashes[hash] = true
    if (!(h.bloom instanceof Uint8Array)) throw new TypeError('invalid argument')
    if (h.bloom.byteLength === 0) filters.push({ numEntries: 0, numBitsPerEntry: 0, numProbes: 0, bits: h.bloom })
    else {
      const pos = { i: 0 }
      const numEntries = readLeb32(h.bloom, pos), numBitsPerEntry = readLeb32(h.bloom, pos), numProbes = readLeb32(h.bloom, pos)
      const n = Math.ceil(numEntries * numBitsPerEntry / 8)
      if (pos.i + n > h.bloom.length) throw new RangeError('subarray exceeds buffer size')
      filters.push({ numEntries, numBitsPerEntry, numProbes, bits: h.bloom.subarray(pos.i, pos.i + n) })
    }
  }
  const list = changesSince(g, Object.keys(lastSyncHashes)), { depFirst, depIndex } = depsOf(g)
  ensureContext(g)
  const listArr = Uint32Array.from(list)
  const inSome = new Uint8Array(list.length)
  for (const f of filters) {
    if (f.numEntries === 0) continue
    const flags = addon.bloomProbe(ctx, listArr, f.numEntries, f.numBitsPerEntry, f.numProbes, f.bits)
    for (let k = 0; k < list.length; k++) inSome[k] |= flags[k]
  }
  const inList = new Set(list), dependents = new Map(), toSend = new Set()
  list.forEach((i, k) => {
    for (let q = depFirst[i]; q < depFirst[i + 1]; q++) {
      const d = depIndex[q]
      if (!dependents.has(d)) dependents.set(d, [])
      dependents.get(d).push(i)
    }
    if (!inSome[k]) toSend.add(i)
  })
  const stack = Array.from(toSend)
  while (stack.length > 0) {
    const i = stack.pop()
    for (const d of dependents.get(i) || []) if (!toSend.has(d)) { toSend.add(d); stack.push(d) }
  }
  const out = []
  for (const hash of need) {
    const i = indexOfHash(g, hash)
    if (i !== undefined) toSend.add(i)
    if (i === undefined || !inList.has(i)) { const change = getChangeByHash(backend, hash); if (change) out.push(change) }
  }
  for (const i of list) if (toSend.has(i)) { engineHashOf.set(g.changes[i], hexOfHash(g, i)); out.push(g.changes[i]) }
  return out
}

// The protocol logic is the REFERENCE'S OWN backend/sync.js, not a restatement of it: a private instance of that file is compiled
// with THIS module as its './backend' (so its Backend.getHeads / getMissingDeps / getChangeByHash / getChanges / applyChanges calls
// land on the functions above -- the bulk receive runs am355_apply_changes) and with two of its module-local functions rebound:
// makeBloomFilter (sync.js:234-238) and getChangesToSend (sync.js:246-306) go to the device paths above when the state is the
// engine's. Its './columnar' is the reference's own with one shortcut: decodeChangeMeta(change, true) of a change the engine
// hashed takes the hash from the engine instead of running SHA-256 in JS again (the reference's own TODO, sync.js:375-377).
// Nothing is written to disk and the instance does not enter require.cache: the installed package keeps its own sync.js.
let boundSyncModule = null
const engineHashOf = new WeakMap()   // change buffer (as retained by a GpuState) -> hex hash the device computed
function boundSync() {
  if (boundSyncModule) return boundSyncModule
  const Module = require('module'), fs = require('fs')
  const dir = path.dirname(require.resolve(process.env.AUTOMERGE_BACKEND_PATH || 'automerge/backend'))
  const file = path.join(dir, 'sync.js')
  const rebind = '\n;module.exports.__rebind = h => { makeBloomFilter = h.makeBloomFilter(makeBloomFilter); getChangesToSend = h.getChangesToSend(getChangesToSend) }\n'
  const realColumnar = columnar()
  const columnarForSync = Object.assign(Object.create(realColumnar), {
    decodeChangeMeta(change, computeHash) {
      const known = computeHash ? engineHashOf.get(change) : undefined
      if (known === undefined) return realColumnar.decodeChangeMeta(change, computeHash)
      const meta = realColumnar.decodeChangeMeta(change, false)
      meta.hash = known
      return meta
    }
  })
  const m = new Module(file, module)
  m.filename = file
  m.paths = Module._nodeModulePaths(dir)
  m.require = function (id) {
    if (id === './backend') return module.exports
    if (id === './columnar') return columnarForSync
    return Module.prototype.require.call(this, id)
  }
  m._compile(fs.readFileSync(file, 'utf8') + rebind, file)
  m.loaded = true
  const engineState = backend => { const g = gpuHistory(backend, true); return g && g.pendingIdx ? g : null }
  m.exports.__rebind({
    makeBloomFilter: original => (backend, lastSync) => {
      const g = engineState(backend)
      return g ? makeBloomFilterGpu(g, lastSync) : original(backend, lastSync)
    },
    getChangesToSend: original => (backend, have, need) => {
      const g = engineState(backend)
      return g ? changesToSendGpu(backend, g, have, need) : original(backend, have, need)
    }
  })
  boundSyncModule = m.exports
  return boundSyncModule
}
const syncModule = () => (JS_ONLY ? ref() : boundSync())

const delegate1 = name => (backend, ...args) => ref()[name](toJs(backend), ...args)

// Backend.getChangesAdded(b1, b2) = BackendDoc(b2).getChangesAdded(BackendDoc(b1)) (backend.js:166-168, new.js:1979-1997; half of
// Automerge.merge) without a BackendDoc of either: the engine walks b2's graph from its heads (am355_changes_added) and stops at the
// hashes b1 has applied. Served when b2 is an engine state with a known history and b1 is one too -- or is empty, as Backend.init()
// makes it: its changeIndexByHash holds nothing. The reference rebuilds the hash graph of b2 (`this`, :1980) and reads b1's index as
// it is: a b1 that began with a loaded document whose graph the reference has not rebuilt knows only the hashes applied since, which
// the wrapper does not track -- such a pair, a state whose queue is held back and a reference-made state keep the hydrating path.
// null: not served.
function gpuChangesAdded(b1, b2) {
  if (JS_ONLY) return null
  const g1 = b1.state instanceof GpuState ? b1.state : null
  if (b1.frozen || b2.frozen || !(g1 ? !g1.js : isEmptyRefState(b1))) return null
  if (g1 && g1.doc && !g1.changes && !g1.noHistory && g1.graphKnown) loadedHistory(g1)
  if (g1 && (heldBack(g1) || !g1.hashes || !g1.applied || ((g1.doc || g1.fromDocument) && !g1.graphKnown))) return null
  const g2 = gpuHistory(b2, true)
  if (!g2) return null
  let other
  if (!g1) other = new Uint8Array(0)
  else if (g1.applied.length * 32 === g1.hashes.length) other = g1.hashes   // (everything applied: in any order)
  else {
    other = new Uint8Array(32 * g1.applied.length)
    g1.applied.forEach((i, k) => other.set(g1.hashes.subarray(32 * i, 32 * i + 32), 32 * k))
  }
  let idx
  try {
    ensureContext(g2)
    idx = addon.changesAdded(ctx, other)
  } catch (e) {
    if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED) throw e
    return null
  }
  noteGraphQuery(b2)   // (new.js:1980: `this` is the state of b2)
  counters.gpuChangesAdded++
  return Array.from(idx, i => g2.changes[i])
}
function getChangesAdded(b1, b2) {
  const served = gpuChangesAdded(b1, b2)
  if (served) return served
  noteGraphQuery(b1)
  return ref().getChangesAdded(hydrate(b1), hydrate(b2))
}

// ---- the string of a Text object: getText / getTextInfo (additions; nothing of backend/index.js:1-8 changes) ----
// What the reference's frontend shows as doc.<path>.toString() / .length after applyPatch(getPatch(state)), without the patch: the
// engine gathers the string from its edit records (am355_object_text) while the state's context is live, the state's queue is not held
// back and the state is the engine's. Otherwise, and for an engine error other than AM355_E_ARG, the JS path: the whole-document patch
// folded by the rule of updateTextObject + toString (frontend/apply_patch.js:231-255, frontend/text.js:64-67; csrc/am355_text.hip):
// one element per index, the last `update` of an index wins, only strings are concatenated, a `remove` splices.
const OBJECT_ID = /^(\d{1,10})@((?:[0-9a-f]{2})+)$/
let textOnEngine = true   // _setTextOnEngine(false): every read takes the JS path (tests, A/B)
function textFromPatch(patch, objectId) {
  let found = null
  const walk = diff => {
    if (found) return
    if (diff.objectId === objectId) { found = diff; return }
    if (diff.props) for (const key of Object.keys(diff.props)) for (const id of Object.keys(diff.props[key])) if (diff.props[key][id].objectId) walk(diff.props[key][id])
    if (diff.edits) for (const e of diff.edits) if (e.value && e.value.objectId) walk(e.value)
  }
  walk(patch.diffs)
  if (!found) throw new RangeError(`no such object: ${objectId}`)
  if (found.type !== 'text') throw new RangeError('not a Text object')
  const elems = [], str = v => (v.objectId === undefined && v.datatype === undefined && typeof v.value === 'string' ? v.value : null)
  for (const e of found.edits) {
    if (e.action === 'insert') elems.splice(e.index, 0, str(e.value))
    else if (e.action === 'multi-insert') for (let k = 0; k < e.values.length; k += 4096) elems.splice(e.index + k, 0, ...e.values.slice(k, k + 4096).map(v => (e.datatype === undefined && typeof v === 'string' ? v : null)))
    else if (e.action === 'update') elems[Math.min(e.index, elems.length)] = str(e.value)
    else if (e.action === 'remove') elems.splice(e.index, e.count)
  }
  const strings = elems.filter(v => v !== null)
  return { text: strings.join(''), length: elems.length, strings: strings.length }
}
function getTextInfo(backend, objectId) {
  isFrozenCheck(backend)
  const g = backend.state
  const m = typeof objectId === 'string' ? OBJECT_ID.exec(objectId) : null
  if (!JS_ONLY && textOnEngine && m && Number(m[1]) <= 0xffffffff && g instanceof GpuState && !heldBack(g) && contextOf(g.generation)) {
    try {
      const r = addon.objectText(ctx, Number(m[1]), new Uint8Array(Buffer.from(m[2], 'hex')))
      counters.gpuText++
      return r
    } catch (e) {
      if (e.am355Code === AM355_E_ARG) throw new RangeError(e.message)
      if (e.am355Code === undefined) throw e
    }
  }
  counters.textFallbacks++
  return textFromPatch(getPatch(backend), objectId)
}
const getText = (backend, objectId) => getTextInfo(backend, objectId).text

// ---- a Text edited by position: spliceText / locateText (additions; nothing of backend/index.js:1-8 changes) ----
// spliceText(backend, objectId, start, deletions, stringOrArrayOfStrings, {actor, time, message}) -> [backend', patch, binaryChange]: one
// context.splice of the reference's frontend (frontend/context.js:441-502; what text.deleteAt / text.insertAt come down to) for a host
// WITHOUT a frontend document. The engine resolves the positions to elemIds and preds on the device, builds the change request the
// frontend would have made and applies it (am355_text_splice) -- while the state's context is live, the state's queue is not held back
// and the state is the engine's. A JS string is split by code point ([...s]), as text.insertAt(i, ...s) does; an array is taken as it
// is, one element per string. Nothing to delete and nothing to insert: [backend, null, null], nothing is applied.
// THE CALLER OWNS THE ACTOR AND THE ORDER OF ITS CALLS: seq is the actor's clock entry + 1 and the deps are the state's heads, as for a
// frontend with nothing in flight. A frontend document that sits on the same backend does not learn of the change by itself.
// Otherwise, and for AM355_E_UNSUPPORTED, the JS path: the whole-document patch folded into (elemId, pred) per element by the rule of
// updateTextObject (frontend/apply_patch.js:231-255: insert -> opId, multi-insert -> the elemId, update -> opId with the elemId kept),
// the request built by context.js's rule, this module's own applyLocalChange. Out of bounds: a RangeError with the reference's text;
// a Counter among the deleted elements: a TypeError with the text of context.js:471 (the reference's frontend itself throws it for
// lists only: for a Text it looks the element up as object[index], finds nothing, and deletes the counter) -- on both paths.
// locateText(backend, objectId, first, n) -> { length, runs: [{ elemId, pred, count, counter }] }: the elements [first, first + n) as the
// runs context.splice would merge into multiOp deletions (am355_text_locate, or the same fold).
let spliceOnEngine = true   // _setSpliceOnEngine(false): every call takes the JS path (tests, A/B)
const COUNTER_IN_TEXT = 'Unsupported operation: deleting a counter from a list'
function elementsFromPatch(patch, objectId) {
  let found = null
  const walk = diff => {
    if (found) return
    if (diff.objectId === objectId) { found = diff; return }
    if (diff.props) for (const key of Object.keys(diff.props)) for (const id of Object.keys(diff.props[key])) if (diff.props[key][id].objectId) walk(diff.props[key][id])
    if (diff.edits) for (const e of diff.edits) if (e.value && e.value.objectId) walk(e.value)
  }
  walk(patch.diffs)
  if (!found) throw new RangeError(`no such object: ${objectId}`)
  if (found.type !== 'text') throw new RangeError('not a Text object')
  const elems = []
  for (const e of found.edits) {
    if (e.action === 'insert') elems.splice(e.index, 0, { elemId: e.elemId, pred: e.opId, counter: e.value.datatype === 'counter' })
    else if (e.action === 'multi-insert') {
      const at = e.elemId.indexOf('@'), ctr = Number(e.elemId.slice(0, at)), actor = e.elemId.slice(at)
      const made = e.values.map((v, k) => ({ elemId: (ctr + k) + actor, pred: (ctr + k) + actor, counter: e.datatype === 'counter' }))
      for (let k = 0; k < made.length; k += 4096) elems.splice(e.index + k, 0, ...made.slice(k, k + 4096))
    } else if (e.action === 'update') elems[e.index] = { elemId: elems[e.index].elemId, pred: e.opId, counter: e.value.datatype === 'counter' }
    else throw new RangeError('a Text element that shows rows but no value: positions through the patch')
  }
  return elems
}
function runsOf(elems) {
  const runs = [], parse = id => { const at = id.indexOf('@'); return [Number(id.slice(0, at)), id.slice(at)] }
  let lastElem = null, lastPred = null
  for (const el of elems) {
    const e = parse(el.elemId), p = parse(el.pred), run = runs[runs.length - 1]
    if (run && lastElem[1] === e[1] && lastElem[0] + 1 === e[0] && lastPred[1] === p[1] && lastPred[0] + 1 === p[0]) {
      run.count++
      run.counter = run.counter || el.counter
    } else runs.push({ elemId: el.elemId, pred: el.pred, count: 1, counter: el.counter })
    lastElem = e; lastPred = p
  }
  return runs
}
const outOfBounds = (start, deletions, length) => new RangeError(`${deletions} deletions starting at index ${start} are out of bounds for list of length ${length}`)
const splitValues = values => (typeof values === 'string' ? [...values] : Array.isArray(values) ? values : values === undefined || values === null ? [] : null)
const engineServesText = (backend, m) => !JS_ONLY && spliceOnEngine && m && Number(m[1]) <= 0xffffffff && backend.state instanceof GpuState && !backend.state.js &&
  !heldBack(backend.state) && contextOf(backend.state.generation)

// [backend', patch, binaryChange] of a positional edit the engine has applied to the context `at` (empty change: nothing was to do)
function positionalResult(backend, at, knownBefore, binaryChange) {
  if (binaryChange.length === 0) return [backend, null, null]
  const patch = materialize(addon.fetchApplyIR(ctx, true))
  const graphFirst = at.docLineage && !knownBefore && !!addon.hashGraphKnown(ctx, -1)
  const result = stateAfterApply(at, [binaryChange], patch, graphFirst)
  const own = hexOfHash(result[0].state, result[0].state.hashes.length / 32 - 1)
  const heads = patch.deps.concat([own]).sort()
  result[0].state.heads = heads
  result[0].heads = heads
  backend.frozen = true
  return [result[0], patch, binaryChange]
}

function gpuSpliceText(backend, m, start, deletions, values, actor, time, message) {
  const at = contextForApply(backend)
  if (!at || at.handed) return null
  const knownBefore = at.docLineage ? !!addon.hashGraphKnown(ctx, -1) : true
  const parts = values.map(v => Buffer.from(v, 'utf8')), off = new Uint32Array(parts.length + 1)
  parts.forEach((b, k) => { off[k + 1] = off[k] + b.length })
  let binaryChange
  try {
    binaryChange = addon.textSplice(ctx, Number(m[1]), new Uint8Array(Buffer.from(m[2], 'hex')), start, deletions, new Uint8Array(Buffer.concat(parts)), off,
      new Uint8Array(Buffer.from(actor, 'hex')), time, new Uint8Array(Buffer.from(message, 'utf8')))
  } catch (e) {
    // out of bounds, no such Text, a counter: decided before the state is touched (am355.h); anything else may have dropped it
    if (e.am355Code !== AM355_E_ARG && !(e.am355Code === AM355_E_INVALID && e.message === COUNTER_IN_TEXT)) at.entry.generation = 0
    throw e
  }
  return positionalResult(backend, at, knownBefore, binaryChange)
}

function spliceText(backend, objectId, start, deletions, values, options = {}) {
  isFrozenCheck(backend)
  const list = splitValues(values), { actor, time = 0, message = '' } = options
  if (!list || !list.every(v => typeof v === 'string')) throw new TypeError('spliceText inserts strings: a string, or an array of strings')
  if (typeof actor !== 'string' || !/^([0-9a-f]{2})+$/.test(actor)) throw new TypeError('spliceText needs the actor id (lowercase hex) in its options')
  if (!Number.isSafeInteger(start) || !Number.isSafeInteger(deletions) || !Number.isSafeInteger(time)) throw new TypeError('start, deletions and time are integers')
  const m = typeof objectId === 'string' ? OBJECT_ID.exec(objectId) : null
  if (start >= 0 && deletions >= 0 && engineServesText(backend, m)) {
    try {
      const result = gpuSpliceText(backend, m, start, deletions, list, actor, time, message)
      if (result) { counters.gpuSplice++; return result }
    } catch (e) {
      if (e.am355Code === AM355_E_ARG) throw new RangeError(e.message)
      if (e.am355Code === AM355_E_INVALID && e.message === COUNTER_IN_TEXT) throw new TypeError(e.message)
      if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED) throw e
    }
  }
  counters.spliceFallbacks++
  const whole = getPatch(backend), elems = elementsFromPatch(whole, objectId)
  if (start < 0 || deletions < 0 || start > elems.length - deletions) throw outOfBounds(start, deletions, elems.length)
  if (deletions === 0 && list.length === 0) return [backend, null, null]
  const ops = []
  for (const run of runsOf(elems.slice(start, start + deletions))) {
    if (run.counter) throw new TypeError(COUNTER_IN_TEXT)
    const op = { action: 'del', obj: objectId, elemId: run.elemId, insert: false, pred: [run.pred] }
    if (run.count > 1) op.multiOp = run.count
    ops.push(op)
  }
  if (list.length > 0) {
    const op = { action: 'set', obj: objectId, elemId: start ? elems[start - 1].elemId : '_head', insert: true }
    if (list.length > 1) op.values = list; else op.value = list[0]
    op.pred = []
    ops.push(op)
  }
  // (the deps are the state's heads; applyLocalChange adds the actor's last hash and keeps every hash once, backend.js:73-81)
  return applyLocalChange(backend, { actor, seq: (whole.clock[actor] || 0) + 1, startOp: whole.maxOp + 1, deps: whole.deps.slice(), time, message, ops })
}

function locateText(backend, objectId, first, n) {
  isFrozenCheck(backend)
  if (!Number.isSafeInteger(first) || !Number.isSafeInteger(n) || first < 0 || n < 0) throw new RangeError('first and n are non-negative integers')
  const m = typeof objectId === 'string' ? OBJECT_ID.exec(objectId) : null
  if (engineServesText(backend, m)) {
    try {
      return addon.textLocate(ctx, Number(m[1]), new Uint8Array(Buffer.from(m[2], 'hex')), first, n)
    } catch (e) {
      if (e.am355Code === AM355_E_ARG) throw new RangeError(e.message)
      if (e.am355Code === undefined) throw e
    }
  }
  const elems = elementsFromPatch(getPatch(backend), objectId)
  if (first + n > elems.length) throw new RangeError(`elements [${first}, ${first} + ${n}) are out of bounds for a Text of length ${elems.length}`)
  return { length: elems.length, runs: runsOf(elems.slice(first, first + n)) }
}

// ---- a plain list edited by position: spliceList / setListItem / locateList (additions; nothing of backend/index.js:1-8 changes) ----
// spliceList(backend, objectId, start, deletions, values, {actor, time, message}) -> [backend', patch, binaryChange]: one context.splice of
// the reference's frontend on a list made by makeList (list.deleteAt / list.insertAt), setListItem(backend, objectId, index, value,
// options): list[index] = value (context.js:411-435; an index at or past the length inserts nulls up to it) -- for a host WITHOUT a
// frontend document, under the conditions of spliceText and with its ownership of actor and order. An element of a list keeps every
// conflicting value: a deletion or an assignment names the op ids of all of them as pred (apply_patch.js:156-213, context.js:576-586).
// A value is a string, a boolean, null, a number (a safe integer is an int, any other a float64, context.js:83-88), a Date (timestamp)
// or { value, datatype } with datatype 'int', 'uint', 'float64', 'counter' or 'timestamp'. Objects cannot be inserted (TypeError).
// Several inserted values that all carry the same datatype are one `set` with `values`, else one inserting `set` per value.
// setListItem ALWAYS makes the op: the reference's frontend skips an assignment of the value the element already shows when there is no
// conflict; this module holds no frontend values to compare -- on both paths.
// Served by the engine (am355_list_splice / am355_list_set / am355_list_locate); otherwise, and on AM355_E_UNSUPPORTED, the JS path: the
// whole-document patch folded into (elemId, preds) per element by the rule of updateListObject, the request built by context.js's rules,
// this module's own applyLocalChange. Out of bounds: a RangeError with the reference's text; a deleted element that shows a Counter: the
// TypeError of context.js:471; an assignment onto one: the RangeError of context.js:422 -- on both paths. A list with an element whose
// first edit is an `update` (the reference's frontend has no elemId for it) is a RangeError on the JS path.
// locateList(backend, objectId, first, n) -> { length, runs: [{ elemId, preds, count, counter }] }.
const COUNTER_ASSIGN = 'Cannot overwrite a Counter object; use .increment() or .decrement() to change its value.'
const LIST_DATATYPES = new Set(['int', 'uint', 'float64', 'counter', 'timestamp'])
function listValue(v) {   // -> { value, datatype } as an op of the reference's frontend carries them
  if (v === null || typeof v === 'string' || typeof v === 'boolean') return { value: v, datatype: undefined }
  if (typeof v === 'number') return { value: v, datatype: Number.isSafeInteger(v) ? 'int' : 'float64' }
  if (v instanceof Date) return { value: v.getTime(), datatype: 'timestamp' }
  if (typeof v === 'object' && !Array.isArray(v) && typeof v.value === 'number' && LIST_DATATYPES.has(v.datatype) && Object.keys(v).length === 2) return { value: v.value, datatype: v.datatype }
  throw new TypeError('a list value is a string, a boolean, null, a number, a Date or { value, datatype }: objects are not inserted by position')
}
function listElementsFromPatch(patch, objectId) {
  let found = null
  const walk = diff => {
    if (found) return
    if (diff.objectId === objectId) { found = diff; return }
    if (diff.props) for (const key of Object.keys(diff.props)) for (const id of Object.keys(diff.props[key])) if (diff.props[key][id].objectId) walk(diff.props[key][id])
    if (diff.edits) for (const e of diff.edits) if (e.value && e.value.objectId) walk(e.value)
  }
  walk(patch.diffs)
  if (!found) throw new RangeError(`no such object: ${objectId}`)
  if (found.type !== 'list') throw new RangeError('not a list object')
  const elems = [], edits = found.edits
  for (let i = 0; i < edits.length; i++) {
    const e = edits[i]
    if (e.action === 'insert' || e.action === 'update') {
      const preds = [e.opId]
      let shown = e.value
      while (i + 1 < edits.length && edits[i + 1].index === e.index && edits[i + 1].action === 'update') { i++; preds.push(edits[i].opId); shown = edits[i].value }
      const counter = shown.datatype === 'counter'
      if (e.action === 'insert') elems.splice(e.index, 0, { elemId: e.elemId, preds, counter })
      else if (e.index < elems.length) elems[e.index] = { elemId: elems[e.index].elemId, preds, counter }   // (behind a multi-insert: the updates replace the conflicts)
      else throw new RangeError('a list element whose first edit is an `update`: the frontend has no elemId for it')
    } else if (e.action === 'multi-insert') {
      const at = e.elemId.indexOf('@'), ctr = Number(e.elemId.slice(0, at)), actor = e.elemId.slice(at)
      const made = e.values.map((v, k) => ({ elemId: (ctr + k) + actor, preds: [(ctr + k) + actor], counter: e.datatype === 'counter' }))
      for (let k = 0; k < made.length; k += 4096) elems.splice(e.index + k, 0, ...made.slice(k, k + 4096))
    } else throw new RangeError('a list element that shows rows but no value: positions through the patch')
  }
  return elems
}
function listRunsOf(elems) {
  const runs = [], parse = id => { const at = id.indexOf('@'); return [Number(id.slice(0, at)), id.slice(at)] }
  let lastElem = null, lastPred = null
  for (const el of elems) {
    const e = parse(el.elemId), p = el.preds.length === 1 ? parse(el.preds[0]) : null, run = runs[runs.length - 1]
    if (run && lastPred && p && lastElem[1] === e[1] && lastElem[0] + 1 === e[0] && lastPred[1] === p[1] && lastPred[0] + 1 === p[0]) {
      run.count++
      run.counter = run.counter || el.counter
    } else runs.push({ elemId: el.elemId, preds: el.preds.slice(), count: 1, counter: el.counter })
    lastElem = e; lastPred = p
  }
  return runs
}
// the ops of context.splice over the folded elements; nextOp: the op number of the first one
function listSpliceOps(elems, objectId, start, deletions, values, actor, nextOp) {
  if (start < 0 || deletions < 0 || start > elems.length - deletions) throw outOfBounds(start, deletions, elems.length)
  const ops = []
  for (const run of listRunsOf(elems.slice(start, start + deletions))) {
    if (run.counter) throw new TypeError(COUNTER_IN_TEXT)
    const op = { action: 'del', obj: objectId, elemId: run.elemId, insert: false, pred: run.preds }
    if (run.count > 1) op.multiOp = run.count
    ops.push(op)
    nextOp += run.count
  }
  let elemId = start ? elems[start - 1].elemId : '_head'
  if (values.length > 1 && values.every(v => v.datatype === values[0].datatype)) {
    const op = { action: 'set', obj: objectId, elemId, insert: true, values: values.map(v => v.value), pred: [] }
    if (values[0].datatype) op.datatype = values[0].datatype
    ops.push(op)
  } else {
    for (const v of values) {
      const op = { action: 'set', obj: objectId, elemId, insert: true, value: v.value, pred: [] }
      if (v.datatype) op.datatype = v.datatype
      ops.push(op)
      elemId = `${nextOp++}@${actor}`
    }
  }
  return ops
}
function listCallArgs(name, objectId, options, numbers) {
  const { actor, time = 0, message = '' } = options
  if (typeof actor !== 'string' || !/^([0-9a-f]{2})+$/.test(actor)) throw new TypeError(`${name} needs the actor id (lowercase hex) in its options`)
  if (!numbers.every(Number.isSafeInteger) || !Number.isSafeInteger(time)) throw new TypeError('positions, counts and time are integers')
  return { actor, time, message, m: typeof objectId === 'string' ? OBJECT_ID.exec(objectId) : null }
}
// one list call on the engine: call(at, idBytes...) -> the binary change; null when the engine does not serve the state
function gpuListEdit(backend, flat, call) {
  const at = contextForApply(backend)
  if (!at || at.handed || !flat) return null
  const knownBefore = at.docLineage ? !!addon.hashGraphKnown(ctx, -1) : true
  let binaryChange
  try {
    binaryChange = call(flat)
  } catch (e) {
    // out of bounds, no such list or map, a bad key, a counter rule: decided before the state is touched (am355.h); anything else may have dropped it
    if (e.am355Code !== AM355_E_ARG && !(e.am355Code === AM355_E_INVALID && (e.message === COUNTER_IN_TEXT || e.message === COUNTER_ASSIGN || e.message === NOT_A_COUNTER))) at.entry.generation = 0
    throw e
  }
  return positionalResult(backend, at, knownBefore, binaryChange)
}
// (counter / serves: the map calls count in their own word and are served for the empty document too, see updateMap)
function listOnEngine(backend, m, flat, call, counter = 'gpuListSplice', serves = engineServesText) {
  if (!serves(backend, m)) return null
  try {
    const result = gpuListEdit(backend, flat, call)
    if (result) counters[counter]++
    return result
  } catch (e) {
    if (e.am355Code === AM355_E_ARG) throw new RangeError(e.message)
    if (e.am355Code === AM355_E_INVALID && (e.message === COUNTER_IN_TEXT || e.message === NOT_A_COUNTER)) throw new TypeError(e.message)
    if (e.am355Code === AM355_E_INVALID && e.message === COUNTER_ASSIGN) throw new RangeError(e.message)
    if (e.am355Code !== AM355_E_INVALID && e.am355Code !== AM355_E_UNSUPPORTED) throw e
    return null
  }
}
const hexBytes = hex => new Uint8Array(Buffer.from(hex, 'hex'))

function spliceList(backend, objectId, start, deletions, values, options = {}) {
  isFrozenCheck(backend)
  if (!Array.isArray(values) && values !== undefined && values !== null) throw new TypeError('spliceList inserts an array of values')
  const list = (values || []).map(listValue)
  const { actor, time, message, m } = listCallArgs('spliceList', objectId, options, [start, deletions])
  if (start >= 0 && deletions >= 0) {
    const served = listOnEngine(backend, m, flattenValues(list), flat => addon.listSplice(ctx, Number(m[1]), hexBytes(m[2]), start, deletions, flat.values, flat.strings,
      hexBytes(actor), time, new Uint8Array(Buffer.from(message, 'utf8'))))
    if (served) return served
  }
  counters.listSpliceFallbacks++
  const whole = getPatch(backend), elems = listElementsFromPatch(whole, objectId)
  const ops = listSpliceOps(elems, objectId, start, deletions, list, actor, whole.maxOp + 1)
  if (ops.length === 0) return [backend, null, null]
  // (the deps are the state's heads; applyLocalChange adds the actor's last hash and keeps every hash once, backend.js:73-81)
  return applyLocalChange(backend, { actor, seq: (whole.clock[actor] || 0) + 1, startOp: whole.maxOp + 1, deps: whole.deps.slice(), time, message, ops })
}

function setListItem(backend, objectId, index, value, options = {}) {
  isFrozenCheck(backend)
  const v = listValue(value)
  const { actor, time, message, m } = listCallArgs('setListItem', objectId, options, [index])
  if (index < 0) throw new RangeError(`A list index must be positive, but you passed ${index}`)
  const served = listOnEngine(backend, m, flattenValues([v]), flat => addon.listSet(ctx, Number(m[1]), hexBytes(m[2]), index, flat.values, flat.strings, hexBytes(actor), time,
    new Uint8Array(Buffer.from(message, 'utf8'))))
  if (served) return served
  counters.listSpliceFallbacks++
  const whole = getPatch(backend), elems = listElementsFromPatch(whole, objectId)
  let ops
  if (index >= elems.length) {   // context.js:416-420
    ops = listSpliceOps(elems, objectId, elems.length, 0, Array(index - elems.length).fill({ value: null, datatype: undefined }).concat([v]), actor, whole.maxOp + 1)
  } else {
    if (elems[index].counter) throw new RangeError(COUNTER_ASSIGN)
    const op = { action: 'set', obj: objectId, elemId: elems[index].elemId, insert: false, value: v.value, pred: elems[index].preds }
    if (v.datatype) op.datatype = v.datatype
    ops = [op]
  }
  return applyLocalChange(backend, { actor, seq: (whole.clock[actor] || 0) + 1, startOp: whole.maxOp + 1, deps: whole.deps.slice(), time, message, ops })
}

function locateList(backend, objectId, first, n) {
  isFrozenCheck(backend)
  if (!Number.isSafeInteger(first) || !Number.isSafeInteger(n) || first < 0 || n < 0) throw new RangeError('first and n are non-negative integers')
  const m = typeof objectId === 'string' ? OBJECT_ID.exec(objectId) : null
  if (engineServesText(backend, m)) {
    try {
      return addon.listLocate(ctx, Number(m[1]), hexBytes(m[2]), first, n)
    } catch (e) {
      if (e.am355Code === AM355_E_ARG) throw new RangeError(e.message)
      if (e.am355Code === undefined) throw e
    }
  }
  const elems = listElementsFromPatch(getPatch(backend), objectId)
  if (first + n > elems.length) throw new RangeError(`elements [${first}, ${first} + ${n}) are out of bounds for a list of length ${elems.length}`)
  return { length: elems.length, runs: listRunsOf(elems.slice(first, first + n)) }
}

// ---- a map edited by key: updateMap / getMapValues / locateMap (additions; nothing of backend/index.js:1-8 changes) ----
// updateMap(backend, objectId, ops, { actor, time, message }) -> [backend', patch, binaryChange]: ONE change on ONE map (or '_root'), what
// Automerge.change(doc, d => { d.a = 1; delete d.b; d.n.increment(2) }) makes, for a host WITHOUT a frontend document, under the
// conditions of spliceList and with its ownership of actor and order. ops: { action: 'set', key, value } (a value as for spliceList),
// { action: 'del', key }, { action: 'inc', key, value: delta }. The pred of each op names every visible value of its key
// (context.js:576-586 getPred); a deletion of a key without a value makes no op, and a call that ends without one returns
// [backend, null, null]. On a Table only { action: 'del', key: rowId } is served. A `set` ALWAYS makes its op (see setListItem).
// A key named twice in one call is a RangeError on both paths (the frontend would name the first op as the second's pred: not built).
// Counters: gpuMap / mapFallbacks count updateMap calls by the path that served them, gpuMapLocate / mapLocateFallbacks the reads.
// Served by the engine (am355_map_update: every key located in one query on the device); otherwise, and on AM355_E_UNSUPPORTED, the JS
// path: the `props` of the whole-document patch folded into preds and the shown value, the request built by context.js's rules
// (:325-346, :351-362, :531-540, :546-573), this module's own applyLocalChange. An empty key assigned: the RangeError of context.js:294;
// an assignment onto a key that shows a Counter: the RangeError of :334; an increment of a key that shows none: the TypeError of :550 --
// on both paths.
// locateMap(backend, objectId, keys) -> [{ counter, child, ids: [opId, ...], values: [...] }] per key, ids ascending (am355_map_locate, or
// the same fold); getMapValues(backend, objectId, keys) -> { key: { opId: value } } with value = { value, datatype? } or { objectId }.
const EMPTY_KEY = 'The key of a map entry must not be an empty string', NOT_A_COUNTER = 'Only counter values can be incremented'
const KEY_TWICE = 'a key named twice in one call (the second op\'s pred would be the first op: not built)'
const ROOT_ID = ['_root', '0', '']   // (the shape of an OBJECT_ID match)
const MOP = { set: 1, del: 2, inc: 3 }
const lamport = id => { const at = id.indexOf('@'); return [Number(id.slice(0, at)), id.slice(at + 1)] }
const lamportAscending = (a, b) => { const x = lamport(a), y = lamport(b); return x[0] - y[0] || (x[1] < y[1] ? -1 : x[1] > y[1] ? 1 : 0) }
function mapFromPatch(patch, objectId) {
  let found = null
  const walk = diff => {
    if (found) return
    if (diff.objectId === objectId) { found = diff; return }
    if (diff.props) for (const key of Object.keys(diff.props)) for (const id of Object.keys(diff.props[key])) if (diff.props[key][id].objectId) walk(diff.props[key][id])
    if (diff.edits) for (const e of diff.edits) if (e.value && e.value.objectId) walk(e.value)
  }
  walk(patch.diffs)
  if (!found) throw new RangeError(`no such object: ${objectId}`)
  if (found.type !== 'map' && found.type !== 'table') throw new RangeError('not a map object')
  return found
}
function locateInPatch(found, key) {
  const held = (found.props && Object.prototype.hasOwnProperty.call(found.props, key) && found.props[key]) || {}
  const ids = Object.keys(held).sort(lamportAscending)
  const values = ids.map(id => (held[id].objectId ? { objectId: held[id].objectId } : held[id].datatype ? { value: held[id].value, datatype: held[id].datatype } : { value: held[id].value }))
  const shown = ids.length ? held[ids[ids.length - 1]] : null
  return { counter: !!shown && shown.datatype === 'counter', child: !!shown && !!shown.objectId, ids, values }
}
// the engine serves a map call: a state it holds, or (for _root) the empty document, which a reset context is
const engineServesMap = (backend, m) => engineServesText(backend, m) || (!JS_ONLY && spliceOnEngine && m === ROOT_ID && isEmptyRefState(backend))
const EMPTY_WHOLE = { clock: {}, deps: [], maxOp: 0, pendingChanges: 0, diffs: { objectId: '_root', type: 'map', props: {} } }
const wholePatch = backend => (isEmptyRefState(backend) ? EMPTY_WHOLE : getPatch(backend))
function mapArgs(objectId) {
  const m = objectId === '_root' ? ROOT_ID : typeof objectId === 'string' ? OBJECT_ID.exec(objectId) : null
  if (!m) throw new RangeError(`no such object: ${objectId}`)
  return m
}
const keyBytes = keys => {
  const parts = keys.map(k => Buffer.from(k, 'utf8')), off = new Uint32Array(parts.length + 1)
  parts.forEach((b, k) => { off[k + 1] = off[k] + b.length })
  return [new Uint8Array(Buffer.concat(parts)), off]
}
function locateMap(backend, objectId, keys) {
  isFrozenCheck(backend)
  if (!Array.isArray(keys) || !keys.every(k => typeof k === 'string')) throw new TypeError('locateMap takes an array of keys')
  const m = mapArgs(objectId)
  if (engineServesText(backend, m)) {   // (an empty document holds no key: the fold below says so without a context)
    try {
      const [bytes, off] = keyBytes(keys)
      const located = addon.mapLocate(ctx, Number(m[1]), hexBytes(m[2]), bytes, off)
      counters.gpuMapLocate++
      return located
    } catch (e) {
      if (e.am355Code === AM355_E_ARG) throw new RangeError(e.message)
      if (e.am355Code === undefined) throw e
    }
  }
  counters.mapLocateFallbacks++
  const found = mapFromPatch(wholePatch(backend), objectId)
  return keys.map(key => locateInPatch(found, key))
}
function getMapValues(backend, objectId, keys) {
  const out = {}
  locateMap(backend, objectId, keys).forEach((hit, k) => {
    out[keys[k]] = {}
    hit.ids.forEach((id, q) => { out[keys[k]][id] = hit.values[q] })
  })
  return out
}
function updateMap(backend, objectId, ops, options = {}) {
  isFrozenCheck(backend)
  if (!Array.isArray(ops) || !ops.every(op => op && MOP[op.action] && typeof op.key === 'string')) throw new TypeError('updateMap takes ops { action: set | del | inc, key, value }')
  const list = ops.map(op => (op.action === 'set' ? listValue(op.value) : null))
  if (!ops.every(op => op.action !== 'inc' || Number.isSafeInteger(op.value))) throw new TypeError('an increment is an integer')
  const { actor, time, message } = listCallArgs('updateMap', objectId, options, [])
  const m = mapArgs(objectId)
  if (new Set(ops.map(op => op.key)).size !== ops.length) throw new RangeError(KEY_TWICE)
  const flat = flattenValues(list.filter(v => v))
  const served = listOnEngine(backend, m, flat, values => {
    const [keys, off] = keyBytes(ops.map(op => op.key))
    const strings = new Uint8Array(keys.length + values.strings.length), vals = Uint32Array.from(values.values), words = new Uint32Array(6 * ops.length)
    strings.set(keys)
    strings.set(values.strings, keys.length)
    for (let k = 0; k < vals.length; k += 6) if (vals[k] === 6) vals[k + 1] += keys.length   // (AM355_LV_UTF8: the values' strings stand behind the keys)
    let nValues = 0
    ops.forEach((op, k) => {
      const delta = op.action === 'inc' ? BigInt.asUintN(64, BigInt(op.value)) : 0n
      words.set([MOP[op.action], off[k], off[k + 1] - off[k], op.action === 'set' ? nValues++ : 0, Number(delta & 0xffffffffn), Number(delta >> 32n)], 6 * k)
    })
    return addon.mapUpdate(ctx, Number(m[1]), hexBytes(m[2]), words, strings, vals, hexBytes(actor), time, new Uint8Array(Buffer.from(message, 'utf8')))
  }, 'gpuMap', engineServesMap)
  if (served) return served
  counters.mapFallbacks++
  const whole = wholePatch(backend), found = mapFromPatch(whole, objectId), out = []
  ops.forEach((op, k) => {
    const hit = locateInPatch(found, op.key), pred = hit.ids.slice().reverse()   // (the conflicts object lists the greatest op id first, apply_patch.js:61)
    if (found.type === 'table' && (op.action !== 'del' || pred.length > 1)) throw new RangeError('on a table object only the deletion of a row is served')
    if (op.action === 'set') {
      if (op.key === '') throw new RangeError(EMPTY_KEY)
      if (hit.counter) throw new RangeError(COUNTER_ASSIGN)
      const o = { action: 'set', obj: objectId, key: op.key, insert: false, value: list[k].value, pred }
      if (list[k].datatype) o.datatype = list[k].datatype
      out.push(o)
    } else if (op.action === 'inc') {
      if (!hit.counter) throw new TypeError(NOT_A_COUNTER)
      out.push({ action: 'inc', obj: objectId, key: op.key, value: op.value, insert: false, pred })
    } else if (pred.length) out.push({ action: 'del', obj: objectId, key: op.key, insert: false, pred })
  })
  if (out.length === 0) return [backend, null, null]
  return applyLocalChange(backend, { actor, seq: (whole.clock[actor] || 0) + 1, startOp: whole.maxOp + 1, deps: whole.deps.slice(), time, message, ops: out })
}

// ---- elemIds of a Text resolved to positions: positionsOfText (an addition; nothing of backend/index.js:1-8 changes) ----
// positionsOfText(backend, objectId, elemIds) -> { length, positions: [{ status: 'visible' | 'deleted' | 'unknown', position, counter }] }: where
// the elements stand NOW -- what keeps a caret, a selection or a comment anchor alive while remote changes arrive. visible: position =
// the element's index; deleted: the element was inserted into this Text and shows no value any more, position = the number of visible
// elements in front of where it stood; unknown: no applied change inserted such an element into this Text (position 0). The caret
// directly behind a known element is position + (status === 'visible').
// Served by the engine (am355_text_position: a search in the stored list order, deleted elements included) under the conditions of
// getText, for a state made of changes; a loaded document that has not been changed yet takes the JS path (the engine would first turn
// its context into the state of the document's rebuilt changes, which this module's bookkeeping of loaded documents does not expect).
// Otherwise, and on AM355_E_UNSUPPORTED, the JS path, slow by design and THE DEFINITION: per element a PROBE on the reference's backend
// -- a change of a fresh actor with startOp = maxOp + 1, deps = heads and the one op {set, insert, elemId, pred: []}, applied to a clone
// of the state; its op id is the greatest, so it lands directly behind the element, and the patch reports it at index = the caret
// position behind it. A probe the reference rejects for a missing reference element gives 'unknown'. An element is visible iff the
// whole-document patch, folded as the frontend folds it, shows it.
let positionOnEngine = true   // _setPositionOnEngine(false): every call takes the JS path (tests, A/B)
const ELEM_ID = /^(\d{1,16})@((?:[0-9a-f]{2})+)$/
const POS_STATUS = ['unknown', 'visible', 'deleted']
function shownElemIds(patch, objectId) {
  let found = null
  const walk = diff => {
    if (found) return
    if (diff.objectId === objectId) { found = diff; return }
    if (diff.props) for (const key of Object.keys(diff.props)) for (const id of Object.keys(diff.props[key])) if (diff.props[key][id].objectId) walk(diff.props[key][id])
    if (diff.edits) for (const e of diff.edits) if (e.value && e.value.objectId) walk(e.value)
  }
  walk(patch.diffs)
  if (!found) throw new RangeError(`no such object: ${objectId}`)
  if (found.type !== 'text') throw new RangeError('not a Text object')
  const elems = []   // { elemId, counter } per index, as updateTextObject builds them (a `remove` splices what is there, as in textFromPatch)
  for (const e of found.edits) {
    if (e.action === 'insert') elems.splice(e.index, 0, { elemId: e.elemId, counter: e.value.datatype === 'counter' })
    else if (e.action === 'multi-insert') {
      const at = e.elemId.indexOf('@'), ctr = Number(e.elemId.slice(0, at)), actor = e.elemId.slice(at)
      const made = e.values.map((v, k) => ({ elemId: (ctr + k) + actor, counter: e.datatype === 'counter' }))
      for (let k = 0; k < made.length; k += 4096) elems.splice(e.index + k, 0, ...made.slice(k, k + 4096))
    } else if (e.action === 'update') { if (elems[e.index]) elems[e.index] = { elemId: elems[e.index].elemId, counter: e.value.datatype === 'counter' } }
    else if (e.action === 'remove') elems.splice(e.index, e.count)
  }
  return elems
}
function probeFallback(backend, objectId, elemIds) {
  const whole = getPatch(backend), shown = new Map(shownElemIds(whole, objectId).map(el => [el.elemId, el.counter]))
  const known = new Set(Object.keys(whole.clock))
  let actor = 'ff'.repeat(16)
  while (known.has(actor)) actor = (BigInt('0x' + actor) - 1n).toString(16).padStart(32, '0')
  const js = hydrate(backend), heads = ref().getHeads(js), opId = `${whole.maxOp + 1}@${actor}`
  const find = diff => {
    if (diff.objectId === objectId) return diff
    if (diff.props) for (const key of Object.keys(diff.props)) for (const id of Object.keys(diff.props[key])) { const d = diff.props[key][id].objectId && find(diff.props[key][id]); if (d) return d }
    if (diff.edits) for (const e of diff.edits) { const d = e.value && e.value.objectId && find(e.value); if (d) return d }
    return null
  }
  const ask = elemId => {
    const probe = columnar().encodeChange({ actor, seq: 1, startOp: whole.maxOp + 1, time: 0, message: '', deps: heads,
      ops: [{ action: 'set', obj: objectId, elemId, insert: true, value: '#', pred: [] }] })
    try {
      return ref().applyChanges(ref().clone(js), [probe])[1]
    } catch (e) {
      return null   // (no such reference element, or an actor the document has never seen)
    }
  }
  // (a Text no element was ever inserted into: the reference finds no op of the object and places the probe without looking for its
  // reference element at all -- it accepts an id nobody issued; there every element is unknown)
  const rowless = shown.size === 0 && known.size > 0 && ask(`${whole.maxOp + 2}@${known.values().next().value}`) !== null
  const positions = elemIds.map(elemId => {
    if (typeof elemId !== 'string' || !ELEM_ID.test(elemId)) throw new TypeError(`not an element id: ${elemId}`)
    const patch = rowless ? null : ask(elemId)
    if (!patch) return { status: 'unknown', position: 0, counter: false }
    const diff = find(patch.diffs), edit = diff && diff.edits.find(x => x.opId === opId)
    if (!edit) throw new Error(`positionsOfText: the probe behind ${elemId} is not in the reference's patch`)
    return shown.has(elemId) ? { status: 'visible', position: edit.index - 1, counter: shown.get(elemId) } : { status: 'deleted', position: edit.index, counter: false }
  })
  return { length: shown.size, positions }
}
function positionsOfText(backend, objectId, elemIds) {
  isFrozenCheck(backend)
  if (!Array.isArray(elemIds)) throw new TypeError('positionsOfText takes an array of element ids')
  const g = backend.state
  const m = typeof objectId === 'string' ? OBJECT_ID.exec(objectId) : null
  if (!JS_ONLY && positionOnEngine && m && Number(m[1]) <= 0xffffffff && g instanceof GpuState && !g.doc && !heldBack(g) && contextOf(g.generation)) {
    try {
      const ids = new Uint32Array(2 * elemIds.length), ranks = new Map()
      elemIds.forEach((elemId, k) => {
        const x = typeof elemId === 'string' ? ELEM_ID.exec(elemId) : null
        if (!x) throw new TypeError(`not an element id: ${elemId}`)
        if (!ranks.has(x[2])) ranks.set(x[2], addon.rankOfActor(ctx, new Uint8Array(Buffer.from(x[2], 'hex'))))
        const rank = ranks.get(x[2]), ctr = Number(x[1])
        const asked = rank >= 0 && ctr <= 0xffffffff   // (an actor the state does not know, a counter no row can hold: unknown)
        ids[2 * k] = asked ? ctr : 0
        ids[2 * k + 1] = asked ? rank : 0xffffffff
      })
      const r = addon.textPositions(ctx, Number(m[1]), new Uint8Array(Buffer.from(m[2], 'hex')), ids)
      counters.gpuPosition++
      const positions = new Array(elemIds.length)
      for (let k = 0; k < elemIds.length; k++) positions[k] = { status: POS_STATUS[r.words[2 * k + 1] & 3], position: r.words[2 * k], counter: (r.words[2 * k + 1] & 0x100) !== 0 }
      return { length: r.length, positions }
    } catch (e) {
      if (e.am355Code === AM355_E_ARG) throw new RangeError(e.message)
      if (e.am355Code !== AM355_E_UNSUPPORTED) throw e
    }
  }
  counters.positionFallbacks++
  return probeFallback(backend, objectId, elemIds)
}

module.exports = {
  init, load, loadChanges, getPatch, getHeads, free, save, getAllChanges, getChanges, getChangeByHash, getMissingDeps,
  clone: backend => { noteGraphQuery(backend); return ref().clone(hydrate(backend)) },
  applyChanges,
  applyLocalChange,
  getChangesAdded,
  // additions: the string of a Text object / {text, length, strings}, read on the device (see above)
  getText, getTextInfo,
  // additions: a Text edited by position / positions resolved to ids, on the device (see above)
  spliceText, locateText,
  // additions: a plain list edited by position / positions resolved to ids and every pred, on the device (see above)
  spliceList, setListItem, locateList,
  // additions: a map edited by key / keys resolved to the op ids and values they hold, on the device (see above)
  updateMap, getMapValues, locateMap,
  // addition: elemIds of a Text resolved to positions, deleted elements included, on the device (see above)
  positionsOfText,
  // sync protocol: the reference's own backend/sync.js bound to this module (boundSync above)
  generateSyncMessage: (...a) => syncModule().generateSyncMessage(...a),
  receiveSyncMessage: (...a) => syncModule().receiveSyncMessage(...a),
  encodeSyncMessage: (...a) => syncModule().encodeSyncMessage(...a),
  decodeSyncMessage: (...a) => syncModule().decodeSyncMessage(...a),
  encodeSyncState: (...a) => syncModule().encodeSyncState(...a),
  decodeSyncState: (...a) => syncModule().decodeSyncState(...a),
  initSyncState: (...a) => syncModule().initSyncState(...a),
  // engine statistics of the last GPU replay (not part of the reference surface)
  _engineStats: () => (addon ? addon.stats(ctx) : null),
  _counters: counters,
  // [calls whose map rows were merged into the stored map table in place, calls that tried and declined], over all contexts
  _residentMapMergeCalls: () => contexts.reduce((s, e) => { const w = addon.residentMapMergeCalls(e.ctx); return [s[0] + w[0], s[1] + w[1]] }, [0, 0]),
  // [calls whose batch made objects and was served without merge_run, calls that tried and declined], over all contexts
  _residentNewObjectCalls: () => contexts.reduce((s, e) => { const w = addon.residentNewObjectCalls(e.ctx); return [s[0] + w[0], s[1] + w[1]] }, [0, 0]),
  // [calls whose counter increments were written into the stored map records in place, calls where that stage declined], over all contexts
  _residentCounterCalls: () => contexts.reduce((s, e) => { const w = addon.residentCounterCalls(e.ctx); return [s[0] + w[0], s[1] + w[1]] }, [0, 0]),
  // [local changes built by one workgroup, requests that found the switch on but lay outside its limits: bulk path], over all contexts
  _localSmallCalls: () => contexts.reduce((s, e) => { const w = addon.localSmallCalls(e.ctx); return [s[0] + w[0], s[1] + w[1]] }, [0, 0]),
  // [membership tests of hash-graph queries answered on the device, by the engine's host index], over all contexts; and the switch
  // between the two (am355_set_graph_probe_min) for every context there is
  _graphQueryCalls: () => contexts.reduce((s, e) => { const w = addon.graphQueryCalls(e.ctx); return [s[0] + w[0], s[1] + w[1]] }, [0, 0]),
  _setGraphProbeMin: n => { graphProbeMin = n; for (const e of contexts) addon.setGraphProbeMin(e.ctx, n) },
  _setTextOnEngine: on => { textOnEngine = !!on },
  _setSpliceOnEngine: on => { spliceOnEngine = !!on },
  _setPositionOnEngine: on => { positionOnEngine = !!on },
  _textFromPatch: textFromPatch,   // (bench_text.js: the JS path's fold by itself)
  _applyProfile: profile,
  _hydrate: hydrate   // (tests: the reference handle of an engine state, made the way the state came to be)
}
