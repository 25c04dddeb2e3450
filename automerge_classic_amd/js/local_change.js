// A change request of the reference's frontend ({actor, seq, startOp, time, message, deps, ops: [...]}, backend/backend.js:54) as the plain
// arrays of am355_local_change (include/am355.h): what addon.applyLocalChange / addon.encodeChange take. The engine expands the ops,
// gives numbers their bytes and encodes the columns on the device; here is only what needs to see JS values:
//   - actor ids -> the change-local actor table (author first, the others in id order, columnar.js:154-157) and their ranks;
//   - keys and strings -> one UTF-8 arena;
//   - a number without datatype -> int when it is a safe integer, else float64 (getNumberTypeAndValue, columnar.js:245);
//   - what the flat form cannot express -> notFlat (the engine answers AM355_E_UNSUPPORTED, the caller runs the reference);
//   - what the reference throws on is passed on as it is (LV_BAD ...) and refused by the engine (AM355_E_INVALID).
'use strict'
const ACTIONS = ['makeMap', 'set', 'makeList', 'del', 'makeText', 'inc', 'makeTable']   // (`link`, numeric actions: not in the flat form)
const LK_STRING = 0, LK_HEAD = 1, LK_ELEM = 2
const LOP_INSERT = 1, LOP_VALUES = 2
const LV = { NULL: 0, FALSE: 1, TRUE: 2, UINT: 3, INT: 4, FLOAT64: 5, UTF8: 6, BYTES: 7, COUNTER: 8, TIMESTAMP: 9, BAD: 15 }
const OP_WORDS = 13, VALUE_WORDS = 6
const NONE32 = 0xffffffff
const NAMED = new Map([['counter', LV.COUNTER], ['timestamp', LV.TIMESTAMP], ['int', LV.INT], ['uint', LV.UINT]])

class NotFlat extends Error {}
const HEX = /^([0-9a-f][0-9a-f])+$/
function hexId(s) {
  if (typeof s !== 'string' || !HEX.test(s)) throw new NotFlat('actor id')
  return s
}
function opId(s) {
  if (typeof s !== 'string') throw new NotFlat('op id')
  const m = /^(\d{1,10})@(.*)$/.exec(s)
  if (!m || Number(m[1]) > NONE32) throw new NotFlat('op id')
  return { ctr: Number(m[1]), actor: hexId(m[2]) }
}

const f64 = new Float64Array(1), f64words = new Uint32Array(f64.buffer)

// one value as the six words of am355_local_value (tag, off, len, pad, payload low, payload high); putString(s) -> [off, len] of the arena
function valueWords(v, datatype, multi, putString) {
  let tag = LV.BAD, off = 0, len = 0, lo = 0, hi = 0
  const isNum = typeof v === 'number'
  if (typeof datatype === 'number') throw new NotFlat('numeric datatype')
  const integer = x => { const big = BigInt.asUintN(64, BigInt(x)); lo = Number(big & 0xffffffffn); hi = Number(big >> 32n) }
  if (multi && (datatype === undefined) === isNum) {
    // (validDatatype, columnar.js:438-444: the reference throws)
  } else if (v === null) tag = LV.NULL
  else if (v === false || v === true) tag = v ? LV.TRUE : LV.FALSE
  else if (typeof v === 'string') { tag = LV.UTF8; [off, len] = putString(v) }
  else if (ArrayBuffer.isView(v)) tag = LV.BYTES
  else if (isNum) {
    const named = NAMED.get(datatype)
    if (named !== undefined) {
      if (Number.isSafeInteger(v) && (datatype !== 'uint' || v >= 0)) { tag = named; integer(v) }
    } else if (datatype !== 'float64' && Number.isSafeInteger(v)) { tag = LV.INT; integer(v) }
    else { tag = LV.FLOAT64; f64[0] = v; lo = f64words[0]; hi = f64words[1] }
  } else throw new NotFlat('value that is no primitive')
  return [tag, off, len, 0, lo, hi]
}

// [{ value, datatype }] as the values and the string arena of am355_list_splice / am355_list_set; null: a value the flat form cannot express
function flattenValues(list) {
  const chunks = [], words = []
  let stringsLen = 0
  const putString = s => {
    const b = Buffer.from(s, 'utf8')
    if (b.toString('utf8') !== s) throw new NotFlat('lone surrogate')
    const off = stringsLen
    chunks.push(b)
    stringsLen += b.length
    return [off, b.length]
  }
  try {
    for (const { value, datatype } of list) words.push(...valueWords(value, datatype, false, putString))
  } catch (e) {
    if (!(e instanceof NotFlat)) throw e
    return null
  }
  const strings = Buffer.concat(chunks, stringsLen)
  return { values: Uint32Array.from(words), strings: new Uint8Array(strings.buffer, strings.byteOffset, strings.length) }
}

function flatten(request) {
  try {
    if (request === null || typeof request !== 'object' || !Array.isArray(request.ops) || !Array.isArray(request.deps)) throw new NotFlat('request')
    if (request.hash !== undefined || request.extraBytes) throw new NotFlat('hash / extraBytes')
    for (const f of ['seq', 'startOp', 'time']) if (!Number.isSafeInteger(request[f])) throw new NotFlat(f)
    if (request.message !== undefined && request.message !== null && typeof request.message !== 'string') throw new NotFlat('message')
    const author = hexId(request.actor)
    const actors = new Set([author])
    const chunks = []
    let stringsLen = 0
    const putString = s => {
      const b = Buffer.from(s, 'utf8')
      if (b.toString('utf8') !== s) throw new NotFlat('lone surrogate')
      const off = stringsLen
      chunks.push(b)
      stringsLen += b.length
      return [off, b.length]
    }
    const ops = new Uint32Array(OP_WORDS * request.ops.length)
    const values = [], preds = [], parsed = []
    const putValue = (v, datatype, multi) => { values.push(...valueWords(v, datatype, multi, putString)) }
    request.ops.forEach((op, i) => {
      if (op === null || typeof op !== 'object') throw new NotFlat('op')
      const action = ACTIONS.indexOf(op.action)
      if (action < 0 || op.child !== undefined) throw new NotFlat('action / child')
      const w = OP_WORDS * i
      ops[w] = action
      let obj = null, elem = null
      if (op.obj === '_root') ops[w + 1] = NONE32
      else { obj = opId(op.obj); actors.add(obj.actor); ops[w + 2] = obj.ctr }
      const insert = !!op.insert
      if (op.key) {
        if (typeof op.key !== 'string') throw new NotFlat('key')
        ops[w + 3] = LK_STRING;
        [ops[w + 4], ops[w + 5]] = putString(op.key)
      } else if (op.elemId === '_head') ops[w + 3] = LK_HEAD
      else if (op.elemId) { ops[w + 3] = LK_ELEM; elem = opId(op.elemId); actors.add(elem.actor); ops[w + 7] = elem.ctr }
      else { ops[w + 3] = LK_STRING; ops[w + 5] = 0 }   // (no key at all: the reference throws)
      if (!Array.isArray(op.pred)) throw new NotFlat('pred')
      const opPreds = op.pred.map(opId)
      for (const p of opPreds) actors.add(p.actor)
      const multiIns = op.action === 'set' && !!op.values && insert
      ops[w + 8] = (insert ? LOP_INSERT : 0) | (multiIns ? LOP_VALUES : 0)
      ops[w + 9] = 1
      ops[w + 10] = values.length / VALUE_WORDS
      if (multiIns) {
        if (!Array.isArray(op.values)) throw new NotFlat('values')
        ops[w + 9] = op.values.length
        for (const v of op.values) putValue(v, op.datatype, true)
      } else if (op.action === 'set' || op.action === 'inc') {
        if (op.value === undefined) values.push(LV.BAD, 0, 0, 0, 0, 0)
        else putValue(op.value, op.datatype, false)
      }
      if (op.action === 'del' && op.multiOp > 1) {
        if (!Number.isInteger(op.multiOp) || op.multiOp >= 2 ** 31 || !elem) throw new NotFlat('multiOp')
        ops[w + 9] = op.multiOp
      }
      ops[w + 11] = preds.length / 2
      ops[w + 12] = opPreds.length
      for (const p of opPreds) preds.push(p.actor, p.ctr)
      parsed.push(obj, elem)
    })
    const table = [author].concat(Array.from(actors).filter(a => a !== author).sort())
    const local = new Map(table.map((a, k) => [a, k]))
    const order = table.slice().sort()
    const actorRank = Uint32Array.from(table, a => order.indexOf(a))
    for (let i = 0; i < request.ops.length; i++) {
      const obj = parsed[2 * i], elem = parsed[2 * i + 1]
      if (obj) ops[OP_WORDS * i + 1] = local.get(obj.actor)
      if (elem) ops[OP_WORDS * i + 6] = local.get(elem.actor)
    }
    const predWords = new Uint32Array(preds.length)
    for (let k = 0; k < preds.length; k += 2) { predWords[k] = local.get(preds[k]); predWords[k + 1] = preds[k + 1] }
    const actorOff = new Uint32Array(table.length + 1)
    table.forEach((a, k) => { actorOff[k + 1] = actorOff[k] + a.length / 2 })
    const deps = Buffer.concat(request.deps.map(h => { if (typeof h !== 'string' || h.length !== 64 || !HEX.test(h)) throw new NotFlat('deps'); return Buffer.from(h, 'hex') }))
    const view = b => new Uint8Array(b.buffer, b.byteOffset, b.length)
    return { seq: request.seq, startOp: request.startOp, time: request.time, notFlat: 0,
      message: view(Buffer.from(request.message || '', 'utf8')), deps: view(deps),
      actorOff, actorRank, actorBytes: view(Buffer.from(table.join(''), 'hex')), strings: view(Buffer.concat(chunks, stringsLen)),
      ops, values: Uint32Array.from(values), preds: predWords }
  } catch (e) {
    if (!(e instanceof NotFlat) && !(e instanceof TypeError) && !(e instanceof RangeError)) throw e
    return { seq: 0, startOp: 0, time: 0, notFlat: 1 }
  }
}

module.exports = { flatten, flattenValues }
