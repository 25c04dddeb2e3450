"""ctypes binding of the C ABI in include/am355.h (the HIP replay engine, csrc/libam355.so).

There is no CPU implementation behind this module: if the HIP library is missing or no MI355X is visible,
constructing an Engine raises.  (tests/emu builds a CPU *emulation* of the kernels for logic tests in the
GPU-less container; it is only ever loaded when a test passes its path explicitly.)
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libam355.so")

AM355_OK = 0
AM355_E_DEVICE, AM355_E_ARG, AM355_E_INVALID, AM355_E_UNSUPPORTED, AM355_E_STATE, AM355_E_NOMEM = -1, -2, -3, -4, -5, -6

FLAG_NAMES = {
    1 << 0: "BAD_MAGIC", 1 << 1: "BAD_CHECKSUM", 1 << 2: "BAD_CHUNK", 1 << 3: "BAD_COLUMNS", 1 << 4: "BAD_LEB", 1 << 5: "BAD_RLE",
    1 << 6: "BAD_ROW", 1 << 7: "UNKNOWN_OBJECT", 1 << 8: "BAD_ELEM", 1 << 9: "BAD_PRED", 1 << 10: "DUP_OPID", 1 << 11: "BAD_COUNTER",
    1 << 12: "UNSUPPORTED", 1 << 13: "OVERFLOW", 1 << 16: "BAD_SEQ", 1 << 17: "UNKNOWN_ACTOR", 1 << 18: "BAD_DEFLATE",
}


class Stats(ctypes.Structure):
    _fields_ = [
        ("n_changes", ctypes.c_uint32), ("n_applied", ctypes.c_uint32), ("n_pending", ctypes.c_uint32),
        ("n_actors", ctypes.c_uint32), ("n_objects", ctypes.c_uint32), ("n_heads", ctypes.c_uint32),
        ("n_ops", ctypes.c_uint64), ("max_op", ctypes.c_uint64), ("raw_bytes", ctypes.c_uint64),
        ("n_map_values", ctypes.c_uint64), ("n_list_elems", ctypes.c_uint64), ("n_edits", ctypes.c_uint64),
        ("ir_bytes", ctypes.c_uint64),
        ("ms_total", ctypes.c_float), ("ms_parse", ctypes.c_float), ("ms_host_schedule", ctypes.c_float),
        ("ms_decode", ctypes.c_float), ("ms_merge", ctypes.c_float), ("ms_order", ctypes.c_float), ("ms_hash_stream", ctypes.c_float),
        ("fast_path", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TextInfo(ctypes.Structure):
    """am355_text_info: list length of the Text, elements that are strings, bytes of the string."""
    _fields_ = [("n_elements", ctypes.c_uint32), ("n_strings", ctypes.c_uint32), ("bytes", ctypes.c_uint64)]


# am355_text_run: a run of consecutive (elemId, pred) pairs of a Text (actors: ranks of the engine's actor table)
TEXT_RUN_DTYPE = np.dtype([("elem_ctr", "<u4"), ("elem_actor", "<u4"), ("pred_ctr", "<u4"), ("pred_actor", "<u4"), ("count", "<u4"), ("flags", "<u4")])
# am355_list_run / am355_list_pred: a run of consecutive elements of a plain list and the preds of its elements
LIST_RUN_DTYPE = np.dtype([("elem_ctr", "<u4"), ("elem_actor", "<u4"), ("count", "<u4"), ("flags", "<u4"), ("pred_first", "<u4"), ("pred_num", "<u4")])
LIST_PRED_DTYPE = np.dtype([("actor", "<u4"), ("ctr", "<u4")])
RUN_COUNTER = 1
ELEM_ID_DTYPE = np.dtype([("ctr", "<u4"), ("actor", "<u4")])              # am355_elem_id
ELEM_POS_DTYPE = np.dtype([("position", "<u4"), ("status", "<u4")])       # am355_elem_pos
POS_UNKNOWN, POS_VISIBLE, POS_DELETED, POS_COUNTER = 0, 1, 2, 0x100       # AM355_POS_*
IR_EDIT_DTYPE = np.dtype([(n, "<u4") for n in ("flags", "index", "id_ctr", "id_actor", "elem_ctr", "elem_actor", "first", "val_tl", "val_off", "pad")])   # am355_ir_edit
EDIT_UPDATE, EDIT_REMOVE = 1, 8                                           # AM355_EDIT_*
IR_MAP_DTYPE = np.dtype([("id_ctr", "<u4"), ("id_actor", "<u4"), ("key_off", "<u4"), ("key_len", "<u4"), ("val_tl", "<u4"), ("val_off", "<u4"), ("flags", "<u4"), ("pad", "<u4"),
                         ("counter", "<i8")])                             # am355_ir_map
MAP_HIT_DTYPE = np.dtype([("first", "<u4"), ("num", "<u4"), ("flags", "<u4"), ("pad", "<u4")])   # am355_map_hit
MAP_OP_DTYPE = np.dtype([("kind", "<u4"), ("key_off", "<u4"), ("key_len", "<u4"), ("value", "<u4"), ("delta", "<i8")])   # am355_map_op
MAP_COUNTER, MAP_CHILD, MAP_EMPTY = 1, 2, 4                               # AM355_MAP_*
MOP_SET, MOP_DELETE, MOP_INC = 1, 2, 3                                    # AM355_MOP_*


def decode_ir_value(val_tl, raw):
    """A primitive value of the record tables (type/length word as in the valLen column, columnar.js:300-329; `raw`: its bytes) as
    (value, datatype): what the reference's patch carries as {value, datatype}."""
    tag = val_tl & 15
    if tag <= 2:
        return (None, False, True)[tag], None
    if tag in (3, 4, 8, 9):
        v, shift = 0, 0
        for b in raw:
            v |= (b & 0x7F) << shift
            shift += 7
        if tag != 3 and raw and raw[-1] & 0x40:
            v -= 1 << shift
        return v, {3: "uint", 4: "int", 8: "counter", 9: "timestamp"}[tag]
    if tag == 5:
        return float(np.frombuffer(bytes(raw), dtype="<f8")[0]), "float64"
    if tag == 6:
        b = bytes(raw)
        return (b[3:] if b[:3] == b"\xef\xbb\xbf" else b).decode("utf-8"), None   # (TextDecoder drops a leading U+FEFF, encoding.js:9-17)
    return bytes(raw), "bytes" if tag == 7 else tag


class EngineError(RuntimeError):
    def __init__(self, code, message, flags=0):
        names = [n for b, n in FLAG_NAMES.items() if flags & b]
        super().__init__(f"am355 error {code}: {message}" + (f" [{'|'.join(names)}]" if names else ""))
        self.code = code
        self.flags = flags
        self.flag_names = names


class InvalidChanges(EngineError):
    """The reference would throw on this input (the JS host re-runs it on the JS path to raise the exact error)."""


class UnsupportedChanges(EngineError):
    """Legal input outside the GPU-served subset (documented in DESIGN.md); the JS host uses the JS path."""


class LocalChange(ctypes.Structure):
    """am355_local_change (include/am355.h): a change request as plain arrays."""
    _fields_ = [
        ("seq", ctypes.c_uint64), ("start_op", ctypes.c_uint64), ("time", ctypes.c_int64),
        ("message", ctypes.c_void_p), ("message_len", ctypes.c_uint32),
        ("deps", ctypes.c_void_p), ("n_deps", ctypes.c_uint32),
        ("n_actors", ctypes.c_uint32), ("actor_off", ctypes.c_void_p), ("actor_bytes", ctypes.c_void_p), ("actor_rank", ctypes.c_void_p),
        ("strings", ctypes.c_void_p), ("strings_len", ctypes.c_uint32),
        ("ops", ctypes.c_void_p), ("n_ops", ctypes.c_uint32),
        ("values", ctypes.c_void_p), ("n_values", ctypes.c_uint32),
        ("preds", ctypes.c_void_p), ("n_preds", ctypes.c_uint32),
        ("not_flat", ctypes.c_uint32),
    ]


_ACTIONS = ("makeMap", "set", "makeList", "del", "makeText", "inc", "makeTable")   # (`link`, numeric actions: not in the flat form)
LK_STRING, LK_HEAD, LK_ELEM = 0, 1, 2
LOP_INSERT, LOP_VALUES = 1, 2
LV_NULL, LV_FALSE, LV_TRUE, LV_UINT, LV_INT, LV_FLOAT64, LV_UTF8, LV_BYTES, LV_COUNTER, LV_TIMESTAMP, LV_BAD = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15
_VALUE_DTYPE = np.dtype([("tag", "<u4"), ("off", "<u4"), ("len", "<u4"), ("pad", "<u4"), ("payload", "<u8")])
_MAX_SAFE = 2 ** 53 - 1


class _NotFlat(Exception):
    pass


def _hex_id(s):
    if not isinstance(s, str) or not s or len(s) % 2 or s != s.lower():
        raise _NotFlat(f"actor id {s!r}")
    try:
        return bytes.fromhex(s)
    except ValueError:
        raise _NotFlat(f"actor id {s!r}")


def _op_id(s):
    if not isinstance(s, str) or "@" not in s:
        raise _NotFlat(f"op id {s!r}")
    ctr, actor = s.split("@", 1)
    if not ctr.isdigit() or int(ctr) >= 2 ** 32:
        raise _NotFlat(f"op id {s!r}")
    return int(ctr), _hex_id(actor)


def flatten_change_request(request):
    """The reference's change request ({actor, seq, startOp, time, message, deps, ops: [...]}, backend.js:54) as the arrays of
    am355_local_change. Returns (LocalChange, keep-alive list). What the flat form cannot express sets not_flat (the engine answers
    AM355_E_UNSUPPORTED); what the reference throws on travels as it is and is refused there (AM355_E_INVALID).
    A number without datatype is an int when it is a safe integer, else a float64 (getNumberTypeAndValue, columnar.js:245)."""
    lc = LocalChange()
    keep = []

    def arr(a):
        keep.append(a)
        return a.ctypes.data if a.size else None

    try:
        if "hash" in request or request.get("extraBytes") is not None:
            raise _NotFlat("hash / extraBytes")
        author = _hex_id(request["actor"])
        actors = {author}
        ops_in = request["ops"]
        strings = bytearray()
        ops = np.zeros((len(ops_in), 13), dtype=np.uint32)
        values, preds, parsed = [], [], []

        def put_string(s):
            try:
                b = s.encode("utf-8")
            except UnicodeEncodeError:
                raise _NotFlat("lone surrogate")
            off = len(strings)
            strings.extend(b)
            return off, len(b)

        def put_value(v, datatype, multi):
            tag, off, ln, payload = LV_BAD, 0, 0, 0
            is_num = isinstance(v, (int, float)) and not isinstance(v, bool)
            if isinstance(datatype, (int, float)) and not isinstance(datatype, bool):
                raise _NotFlat("numeric datatype")
            if multi and ((datatype is None) == is_num or (datatype is not None and not is_num)):
                pass   # (validDatatype, columnar.js:438-444: the reference throws)
            elif v is None:
                tag = LV_NULL
            elif v is False or v is True:
                tag = LV_TRUE if v else LV_FALSE
            elif isinstance(v, str):
                tag = LV_UTF8
                off, ln = put_string(v)
            elif isinstance(v, (bytes, bytearray, memoryview)):
                tag = LV_BYTES
            elif is_num:
                whole = isinstance(v, int) or (v == v and abs(v) != float("inf") and float(v).is_integer())
                if datatype in ("counter", "timestamp", "int", "uint"):
                    if whole and abs(int(v)) <= _MAX_SAFE and (datatype != "uint" or int(v) >= 0):
                        tag = {"counter": LV_COUNTER, "timestamp": LV_TIMESTAMP, "int": LV_INT, "uint": LV_UINT}[datatype]
                        payload = int(v) & 0xFFFFFFFFFFFFFFFF
                elif datatype != "float64" and whole and abs(int(v)) <= _MAX_SAFE:
                    tag, payload = LV_INT, int(v) & 0xFFFFFFFFFFFFFFFF
                else:
                    tag, payload = LV_FLOAT64, int(np.array([float(v)], dtype="<f8").view("<u8")[0])
            else:
                raise _NotFlat("value that is no primitive")
            values.append((tag, off, ln, 0, payload))

        for i, op in enumerate(ops_in):
            action = op.get("action")
            if action not in _ACTIONS or "child" in op:
                raise _NotFlat(f"action {action!r} / child")
            r = ops[i]
            r[0] = _ACTIONS.index(action)
            if op["obj"] == "_root":
                obj = None
                r[1] = 0xFFFFFFFF
            else:
                obj = _op_id(op["obj"])
                actors.add(obj[1])
                r[2] = obj[0]
            insert = bool(op.get("insert"))
            elem = None
            if op.get("key"):
                if not isinstance(op["key"], str):
                    raise _NotFlat("key")
                r[3] = LK_STRING
                r[4], r[5] = put_string(op["key"])
            elif op.get("elemId") == "_head":
                r[3] = LK_HEAD
            elif op.get("elemId"):
                r[3] = LK_ELEM
                elem = _op_id(op["elemId"])
                actors.add(elem[1])
                r[7] = elem[0]
            else:
                r[3], r[5] = LK_STRING, 0   # (no key at all: the reference throws)
            if not isinstance(op.get("pred"), list):
                raise _NotFlat("pred")
            op_preds = [_op_id(p) for p in op["pred"]]
            for _, a in op_preds:
                actors.add(a)
            multi_ins = action == "set" and insert and op.get("values") is not None
            r[8] = (LOP_INSERT if insert else 0) | (LOP_VALUES if multi_ins else 0)
            r[9] = 1
            r[10] = len(values)
            if multi_ins:
                if not isinstance(op["values"], list):
                    raise _NotFlat("values")
                r[9] = len(op["values"])
                for v in op["values"]:
                    put_value(v, op.get("datatype"), True)
            elif action in ("set", "inc"):
                if "value" not in op:
                    values.append((LV_BAD, 0, 0, 0, 0))
                else:
                    put_value(op["value"], op.get("datatype"), False)
            if action == "del" and isinstance(op.get("multiOp"), (int, float)) and op["multiOp"] > 1:
                if int(op["multiOp"]) != op["multiOp"] or op["multiOp"] >= 2 ** 31 or elem is None:
                    raise _NotFlat("multiOp")
                r[9] = int(op["multiOp"])
            r[11], r[12] = len(preds), len(op_preds)
            preds.extend(op_preds)
            parsed.append((obj, elem))
        others = sorted(actors - {author})
        table = [author] + others
        local = {a: k for k, a in enumerate(table)}
        order = sorted(table)
        rank = np.array([order.index(a) for a in table], dtype=np.uint32)
        for r, (obj, elem) in zip(ops, parsed):
            if obj is not None:
                r[1] = local[obj[1]]
            if elem is not None:
                r[6] = local[elem[1]]
        pred_arr = np.array([(local[a], ctr) for ctr, a in preds], dtype=np.uint32).reshape(-1, 2)
        val_arr = np.array(values, dtype=_VALUE_DTYPE) if values else np.zeros(0, dtype=_VALUE_DTYPE)
        message = (request.get("message") or "").encode("utf-8")
        deps = np.frombuffer(b"".join(bytes.fromhex(h) for h in request["deps"]), dtype=np.uint8).copy()
        if deps.size != 32 * len(request["deps"]):
            raise _NotFlat("deps")
        for f in ("seq", "startOp", "time"):
            if not isinstance(request[f], int) or isinstance(request[f], bool) or abs(request[f]) >= 2 ** 63:
                raise _NotFlat(f)
        if request["seq"] < 0 or request["startOp"] < 0:
            raise _NotFlat("seq / startOp")
    except (_NotFlat, KeyError, TypeError, ValueError, AttributeError, UnicodeEncodeError):
        lc.not_flat = 1
        return lc, keep
    lc.seq, lc.start_op, lc.time = request["seq"], request["startOp"], request["time"]
    msg = np.frombuffer(message, dtype=np.uint8).copy()
    lc.message, lc.message_len = arr(msg), msg.size
    lc.deps, lc.n_deps = arr(deps), deps.size // 32
    offs = np.zeros(len(table) + 1, dtype=np.uint32)
    np.cumsum([len(a) for a in table], out=offs[1:])
    lc.n_actors = len(table)
    lc.actor_off = arr(offs)
    lc.actor_bytes = arr(np.frombuffer(b"".join(table), dtype=np.uint8).copy())
    lc.actor_rank = arr(rank)
    st = np.frombuffer(bytes(strings), dtype=np.uint8).copy()
    lc.strings, lc.strings_len = arr(st), st.size
    ops = np.ascontiguousarray(ops)
    lc.ops, lc.n_ops = arr(ops), ops.shape[0]
    lc.values, lc.n_values = arr(val_arr), val_arr.size
    lc.preds, lc.n_preds = arr(pred_arr), pred_arr.shape[0]
    return lc, keep


def _bind(path):
    if not os.path.exists(path):
        raise RuntimeError(f"HIP engine library not found: {path}. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = ctypes.CDLL(path)
    vp, u32, u64p = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p
    L.am355_create.restype = vp
    L.am355_create.argtypes = [ctypes.c_int]
    L.am355_destroy.argtypes = [vp]
    L.am355_last_error.restype = ctypes.c_char_p
    L.am355_last_error.argtypes = [vp]
    L.am355_flags.restype = u32
    L.am355_flags.argtypes = [vp]
    L.am355_load_changes.argtypes = [vp, vp, u64p, u32]
    L.am355_load_document.argtypes = [vp, vp, ctypes.c_size_t]
    if hasattr(L, "am355_backend_load"):   # (tools/ab_libs.sh loads libraries of earlier rounds, which end before this entry point; tests/test_abi.py holds the shipped library to the header)
        L.am355_backend_load.argtypes = [vp, vp, ctypes.c_size_t]
        L.am355_backend_load.restype = ctypes.c_int
    L.am355_replay.argtypes = [vp]
    L.am355_patch_json.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t)]
    L.am355_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    L.am355_get_hashes.argtypes = [vp, vp]
    L.am355_test_sort.argtypes = [vp, vp, vp, u32, ctypes.c_int]
    L.am355_test_scan.argtypes = [vp, vp, vp, u32, vp]
    sz, ci = ctypes.c_size_t, ctypes.c_int
    for f, args in (("am355_test_scan_at", [vp, vp, u32, u32, vp, u32, u32, u32, vp]), ("am355_test_scan2", [vp, vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, vp]),
                    ("am355_test_scan_terminators", [vp, vp, sz, u32, u32, vp, u32, u32, vp]), ("am355_test_max", [vp, vp, u32, vp]),
                    ("am355_test_sort_bits", [vp, vp, vp, u32, ci, ci, vp, ctypes.POINTER(ci)]), ("am355_test_chain_mark", [vp, vp, vp, u32, u32]),
                    ("am355_test_remap", [vp, vp, u32, u32, vp, u32, vp, u32, ctypes.POINTER(u32)]), ("am355_test_fill", [vp, vp, u32, u32, vp, u32, ctypes.POINTER(u32)]),
                    ("am355_test_copy", [vp, vp, sz, vp, sz, ci, vp, u32, ctypes.POINTER(u32)]), ("am355_test_signal_words", [vp, vp, u32, vp, u32, u32, vp, u32, vp]),
                    ("am355_test_carried_scan", [vp, vp, u32, vp, vp, vp]), ("am355_test_text_premises", [vp, vp, u32, u32, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)])):
        if not hasattr(L, f):   # (a library of an earlier commit, loaded for an A/B run)
            continue
        getattr(L, f).argtypes = args
        getattr(L, f).restype = ci
    L.am355_get_rows.argtypes = [vp] * 15
    L.am355_save.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    L.am355_get_applied.argtypes = [vp, vp, ctypes.POINTER(u32)]
    L.am355_fetch_ir.argtypes = [vp, vp]
    L.am355_set_shard.argtypes = [vp, u32, u32]
    L.am355_fragment_size.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    L.am355_export_fragment.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    L.am355_import_fragments.argtypes = [vp, vp, vp, u32]
    L.am355_shard_unique_id.argtypes = [vp]
    L.am355_shard_init.argtypes = [vp, vp, u32, u32]
    L.am355_sharded_replay.argtypes = [vp, ctypes.c_int]
    L.am355_shard_fragment_bytes.argtypes = [vp, vp, u32]
    L.am355_shard_finalize.argtypes = [vp]
    for f in ("am355_shard_unique_id", "am355_shard_init", "am355_sharded_replay", "am355_shard_fragment_bytes", "am355_shard_finalize"):
        getattr(L, f).restype = ctypes.c_int
    if hasattr(L, "am355_resident_counters"):   # (tools/ab_apply.sh loads libraries of earlier commits; tests/test_abi.py holds the shipped one to the header)
        L.am355_resident_counters.argtypes = [vp, vp]
        L.am355_resident_counters.restype = ctypes.c_int
    if hasattr(L, "am355_resident_maps_only_calls"):
        L.am355_resident_maps_only_calls.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
        L.am355_resident_maps_only_calls.restype = ctypes.c_int
    if hasattr(L, "am355_set_resident_new_actors"):
        L.am355_set_resident_new_actors.argtypes = [vp, ctypes.c_int]
        L.am355_set_resident_new_actors.restype = ctypes.c_int
        L.am355_resident_new_actor_calls.argtypes = [vp, vp]
        L.am355_resident_new_actor_calls.restype = ctypes.c_int
    if hasattr(L, "am355_set_resident_new_objects"):
        L.am355_set_resident_new_objects.argtypes = [vp, ctypes.c_int]
        L.am355_set_resident_new_objects.restype = ctypes.c_int
        L.am355_resident_new_object_calls.argtypes = [vp, vp]
        L.am355_resident_new_object_calls.restype = ctypes.c_int
    if hasattr(L, "am355_set_resident_counters"):
        L.am355_set_resident_counters.argtypes = [vp, ctypes.c_int]
        L.am355_set_resident_counters.restype = ctypes.c_int
        L.am355_resident_counter_calls.argtypes = [vp, vp]
        L.am355_resident_counter_calls.restype = ctypes.c_int
    if hasattr(L, "am355_set_resident_map_merge"):
        L.am355_set_resident_map_merge.argtypes = [vp, ctypes.c_int]
        L.am355_set_resident_map_merge.restype = ctypes.c_int
        L.am355_resident_map_merge_calls.argtypes = [vp, vp]
        L.am355_resident_map_merge_calls.restype = ctypes.c_int
    if hasattr(L, "am355_apply_local_change"):   # (libraries of earlier commits, loaded for an A/B run, end before these)
        L.am355_encode_change.argtypes = [vp, ctypes.POINTER(LocalChange), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), vp]
        L.am355_apply_local_change.argtypes = [vp, ctypes.POINTER(LocalChange), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.am355_local_change_calls.argtypes = [vp, vp]
        for f in ("am355_encode_change", "am355_apply_local_change", "am355_local_change_calls"):
            getattr(L, f).restype = ctypes.c_int
    if hasattr(L, "am355_set_local_small"):   # (libraries of earlier commits, loaded for an A/B run, end before these)
        L.am355_set_local_small.argtypes = [vp, ctypes.c_int]
        L.am355_set_local_small.restype = ctypes.c_int
        L.am355_local_small_calls.argtypes = [vp, vp]
        L.am355_local_small_calls.restype = ctypes.c_int
    if hasattr(L, "am355_changes_added"):   # (libraries of earlier commits, loaded for an A/B run, end before these)
        L.am355_find_changes.argtypes = [vp, vp, u32, vp]
        for f in ("am355_changes_since", "am355_changes_added", "am355_missing_deps"):
            getattr(L, f).argtypes = [vp, vp, u32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u32)]
        L.am355_set_graph_probe_min.argtypes = [vp, u32]
        L.am355_graph_query_calls.argtypes = [vp, vp]
        L.am355_test_hash_probe.argtypes = [vp, vp, u32, vp, u32, vp]
        for f in ("am355_find_changes", "am355_changes_since", "am355_changes_added", "am355_missing_deps", "am355_set_graph_probe_min", "am355_graph_query_calls",
                  "am355_test_hash_probe"):
            getattr(L, f).restype = ctypes.c_int
    if hasattr(L, "am355_object_text"):   # (libraries of earlier commits, loaded for an A/B run, end before these)
        L.am355_object_text.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(TextInfo)]
        L.am355_object_text_calls.argtypes = [vp, vp]
        L.am355_set_text_pinned_max.argtypes = [vp, ctypes.c_uint64]
        L.am355_text_limits.argtypes = [vp]
        for f in ("am355_object_text", "am355_object_text_calls", "am355_set_text_pinned_max", "am355_text_limits"):
            getattr(L, f).restype = ctypes.c_int
    if hasattr(L, "am355_text_splice"):   # (libraries of earlier commits, loaded for an A/B run, end before these)
        L.am355_text_locate.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u32),
                                        ctypes.POINTER(ctypes.c_uint64)]
        L.am355_text_splice.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, vp, vp, u32, vp, ctypes.c_size_t, ctypes.c_int64, vp, u32,
                                        ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.am355_text_splice_calls.argtypes = [vp, vp]
        L.am355_text_locate_limits.argtypes = [vp]
        for f in ("am355_text_locate", "am355_text_splice", "am355_text_splice_calls", "am355_text_locate_limits"):
            getattr(L, f).restype = ctypes.c_int
    if hasattr(L, "am355_list_splice"):   # (libraries of earlier commits, loaded for an A/B run, end before these)
        pvp, psz = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)
        L.am355_list_locate.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, pvp, ctypes.POINTER(u32), pvp, ctypes.POINTER(u32),
                                        ctypes.POINTER(ctypes.c_uint64)]
        L.am355_list_splice.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint64, vp, u32, vp, u32, vp, ctypes.c_size_t, ctypes.c_int64, vp, u32,
                                        pvp, psz]
        L.am355_list_set.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, ctypes.c_uint64, vp, vp, u32, vp, ctypes.c_size_t, ctypes.c_int64, vp, u32, pvp, psz]
        L.am355_list_splice_calls.argtypes = [vp, vp]
        L.am355_list_locate_limits.argtypes = [vp]
        L.am355_test_list_premises.argtypes = [vp, vp, u32, u32, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
        for f in ("am355_list_locate", "am355_list_splice", "am355_list_set", "am355_list_splice_calls", "am355_list_locate_limits", "am355_test_list_premises"):
            getattr(L, f).restype = ctypes.c_int
    if hasattr(L, "am355_text_position"):   # (libraries of earlier commits, loaded for an A/B run, end before these)
        L.am355_text_position.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, vp, u32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        L.am355_rank_of_actor.argtypes = [vp, vp, ctypes.c_size_t, ctypes.POINTER(u32)]
        L.am355_actor_of_rank.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
        L.am355_actor_of_rank.restype = ctypes.c_int
        L.am355_text_position_calls.argtypes = [vp, vp]
        L.am355_text_position_limits.argtypes = [vp]
        for f in ("am355_text_position", "am355_rank_of_actor", "am355_text_position_calls", "am355_text_position_limits"):
            getattr(L, f).restype = ctypes.c_int
    if hasattr(L, "am355_map_update"):   # (libraries of earlier commits, loaded for an A/B run, end before these)
        pvp, psz = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)
        L.am355_map_locate.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, vp, vp, u32, pvp, pvp, ctypes.POINTER(u32)]
        L.am355_map_update.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_size_t, vp, u32, vp, u32, vp, u32, vp, ctypes.c_size_t, ctypes.c_int64, vp, u32, pvp, psz]
        L.am355_map_calls.argtypes = [vp, vp]
        L.am355_map_locate_limits.argtypes = [vp]
        L.am355_set_map_locate_thread.argtypes = [vp, ctypes.c_int]
        for f in ("am355_map_locate", "am355_map_update", "am355_map_calls", "am355_map_locate_limits", "am355_set_map_locate_thread"):
            getattr(L, f).restype = ctypes.c_int
    L.am355_get_raw.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u32)]
    L.am355_doc_changes.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_void_p)]
    L.am355_apply_changes.argtypes = [vp, vp, u64p, u32]
    L.am355_apply_patch_json.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t)]
    L.am355_fetch_apply_ir.argtypes = [vp, vp]
    L.am355_reset.argtypes = [vp]
    L.am355_get_dep_graph.argtypes = [vp, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(u32)]
    L.am355_sync_bloom_build.argtypes = [vp, vp, u32, vp, ctypes.c_size_t]
    L.am355_sync_bloom_probe.argtypes = [vp, vp, u32, u32, u32, u32, vp, ctypes.c_size_t, vp]
    L.am355_get_pending.argtypes = [vp, vp, ctypes.POINTER(u32)]
    L.am355_forget_call_history.argtypes = [vp, ctypes.c_int]
    L.am355_hash_graph_known.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.am355_set_phase_events.argtypes = [vp, ctypes.c_int]
    for f in ("am355_load_changes", "am355_load_document", "am355_replay", "am355_patch_json", "am355_get_stats", "am355_get_hashes", "am355_test_sort",
              "am355_test_scan", "am355_get_rows", "am355_save", "am355_get_applied", "am355_fetch_ir", "am355_get_raw", "am355_set_shard", "am355_fragment_size", "am355_export_fragment",
              "am355_import_fragments", "am355_doc_changes", "am355_apply_changes", "am355_apply_patch_json", "am355_fetch_apply_ir", "am355_reset", "am355_get_pending", "am355_forget_call_history", "am355_hash_graph_known", "am355_set_phase_events", "am355_get_dep_graph", "am355_sync_bloom_build", "am355_sync_bloom_probe"):
        getattr(L, f).restype = ctypes.c_int
    return L


_libs = {}


def load_library(path=DEFAULT_LIB):
    if path not in _libs:
        _libs[path] = _bind(path)
    return _libs[path]


class Engine:
    """One replay context bound to one GPU (am355_ctx)."""

    def __init__(self, device=0, lib_path=DEFAULT_LIB):
        self._L = load_library(lib_path)
        self.device = device
        self.lib_path = lib_path
        self._h = self._L.am355_create(device)
        if not self._h:
            raise RuntimeError("am355_create failed: no usable MI355X / HIP device (the engine has no CPU fallback)")
        self._n_changes = 0

    def set_phase_events(self, on):
        """Measurement switch (am355_set_phase_events): HIP events between the phases of the following replays."""
        self._check(self._L.am355_set_phase_events(self._h, 1 if on else 0))

    def close(self):
        if getattr(self, "_h", None):
            self._L.am355_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == AM355_OK:
            return
        msg = self._L.am355_last_error(self._h).decode("utf-8", "replace")
        flags = self._L.am355_flags(self._h)
        cls = InvalidChanges if rc == AM355_E_INVALID else UnsupportedChanges if rc == AM355_E_UNSUPPORTED else EngineError
        raise cls(rc, msg, flags)

    # ---- the path -------------------------------------------------------------------------------------
    def load_changes(self, log):
        """Stage a batch (host inflate of DEFLATEd changes + copy to HBM). `log` has .arena (uint8) and .offsets (uint64)."""
        arena = np.ascontiguousarray(log.arena, dtype=np.uint8)
        offsets = np.ascontiguousarray(log.offsets, dtype=np.uint64)
        self._n_changes = int(offsets.size - 1)
        self._check(self._L.am355_load_changes(self._h, arena.ctypes.data if arena.size else None, offsets.ctypes.data, self._n_changes))

    def load_document(self, doc: bytes):
        """Stage one saved document (Backend.save bytes): host header parse / checksum / inflate, op columns to HBM."""
        buf = np.frombuffer(bytes(doc), dtype=np.uint8)
        self._n_changes = 0
        self._check(self._L.am355_load_document(self._h, buf.ctypes.data, buf.size))

    def backend_load(self, doc: bytes):
        """Backend.load(bytes) in one call (am355_backend_load): load_document + replay with the chunk checksum on a thread beside the
        device stages and the patch IR on its way to the host when the call returns."""
        buf = doc if isinstance(doc, np.ndarray) else np.frombuffer(bytes(doc), dtype=np.uint8)
        self._n_changes = 0
        self._check(self._L.am355_backend_load(self._h, buf.ctypes.data, buf.size))

    def replay(self):
        """The hot path: decode + schedule + merge + patch IR, device-resident in and out."""
        self._check(self._L.am355_replay(self._h))

    def apply_changes(self, log):
        """Backend.applyChanges(state, changes): the state is what the context holds (earlier load_changes + replay or apply_changes
        calls, or nothing = Backend.init()). Replays everything, derives the incremental patch of the batch on the device."""
        arena = np.ascontiguousarray(log.arena, dtype=np.uint8)
        offsets = np.ascontiguousarray(log.offsets, dtype=np.uint64)
        self._check(self._L.am355_apply_changes(self._h, arena.ctypes.data if arena.size else None, offsets.ctypes.data, int(offsets.size - 1)))
        self._n_changes = int(self.stats().n_changes)

    def encode_change(self, request):
        """encodeChange(request) (columnar.js:710-739) with the deps as given, the op columns encoded on the device: (bytes, hash).
        Nothing of the state is read or touched. `request`: the reference's change request, see flatten_change_request."""
        lc, keep = flatten_change_request(request)
        p, n, h = ctypes.c_void_p(), ctypes.c_size_t(), (ctypes.c_uint8 * 32)()
        self._check(self._L.am355_encode_change(self._h, ctypes.byref(lc), ctypes.byref(p), ctypes.byref(n), h))
        del keep
        return ctypes.string_at(p, n.value), bytes(h)

    def apply_local_change(self, request):
        """Backend.applyLocalChange(state, request) (backend.js:54-91): returns the binary change; apply_patch_json() then gives the patch.
        InvalidChanges where the reference throws, UnsupportedChanges for what is left to the JS path (include/am355.h)."""
        lc, keep = flatten_change_request(request)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.am355_apply_local_change(self._h, ctypes.byref(lc), ctypes.byref(p), ctypes.byref(n)))
        del keep
        self._n_changes = int(self.stats().n_changes)
        return ctypes.string_at(p, n.value)

    def local_change_calls(self):
        """(requests apply_local_change served, requests it refused)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_local_change_calls(self._h, out))
        return int(out[0]), int(out[1])

    def set_local_small(self, on):
        """am355_set_local_small: a change request inside the limits of csrc/am355_hist.h LOCAL_SMALL_* (a keystroke, a pasted line) is
        built by one workgroup in one launch instead of by the bulk encoders (off by default)."""
        self._check(self._L.am355_set_local_small(self._h, 1 if on else 0))

    def local_small_calls(self):
        """(changes the one workgroup built, requests that found the switch on but lay outside its limits and took the bulk path)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_local_small_calls(self._h, out))
        return int(out[0]), int(out[1])

    def reset(self):
        """Forget the state: the next apply_changes starts from Backend.init()."""
        self._check(self._L.am355_reset(self._h))
        self._n_changes = 0

    def forget_call_history(self, doc_changes=0):
        """The staged changes were replayed in one go, not by the Backend.applyChanges calls that built the state; doc_changes: how
        many of the leading ones are the rebuilt history of a loaded document (include/am355.h)."""
        self._check(self._L.am355_forget_call_history(self._h, int(doc_changes)))

    def hash_graph_known(self, set_to=None):
        """Lineage that began with a loaded document: has the reference rebuilt the document's hash graph (include/am355.h)?
        set_to True / False tells the engine; returns the state afterwards."""
        known = ctypes.c_int(0)
        self._check(self._L.am355_hash_graph_known(self._h, -1 if set_to is None else (1 if set_to else 0), ctypes.byref(known)))
        return bool(known.value)

    def pending(self):
        """Indexes (into the engine's list of changes) of the changes still queued for a missing dependency."""
        n = ctypes.c_uint32()
        self._check(self._L.am355_get_pending(self._h, None, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self._check(self._L.am355_get_pending(self._h, out.ctypes.data, ctypes.byref(n)))
        return out

    # ---- sync protocol, bulk side ----------------------------------------------------------
    def dep_graph(self):
        """(dep_first[n + 1], dep_index[]) over the context's list of changes: change i depends on dep_index[dep_first[i]:dep_first[i + 1]]
        (0xffffffff: a change the context does not hold)."""
        f, x, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        self._check(self._L.am355_get_dep_graph(self._h, ctypes.byref(f), ctypes.byref(x), ctypes.byref(n)))
        first = np.ctypeslib.as_array(ctypes.cast(f, ctypes.POINTER(ctypes.c_uint32)), shape=(n.value + 1,)).copy()
        m = int(first[-1])
        index = np.ctypeslib.as_array(ctypes.cast(x, ctypes.POINTER(ctypes.c_uint32)), shape=(m,)).copy() if m else np.zeros(0, np.uint32)
        return first, index

    def bloom_build(self, idx):
        """`bits` of the sync protocol's Bloom filter (sync.js:38-128) over the hashes of the changes idx[], built on the device."""
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        out = np.zeros((idx.size * 10 + 7) // 8, dtype=np.uint8)
        self._check(self._L.am355_sync_bloom_build(self._h, idx.ctypes.data if idx.size else None, idx.size, out.ctypes.data, out.size))
        return out

    def bloom_probe(self, idx, num_entries, bits_per_entry, num_probes, bits):
        """contains[k] for the hashes of the changes idx[] in a filter received from a peer."""
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        out = np.zeros(max(idx.size, 1), dtype=np.uint8)
        self._check(self._L.am355_sync_bloom_probe(self._h, idx.ctypes.data if idx.size else None, idx.size, num_entries, bits_per_entry, num_probes,
                                                   bits.ctypes.data if bits.size else None, bits.size, out.ctypes.data))
        return out[:idx.size]

    # ---- hash-graph queries over the applied changes (include/am355.h) -------------------------------------
    @staticmethod
    def _hash_rows(hashes):
        """A list of 32-byte hashes (bytes or hex strings), or an (n, 32) array, as one contiguous (n, 32) uint8 array."""
        if isinstance(hashes, np.ndarray):
            a = np.ascontiguousarray(hashes, dtype=np.uint8).reshape(-1, 32)
        else:
            a = np.frombuffer(b"".join(bytes.fromhex(h) if isinstance(h, str) else bytes(h) for h in hashes), dtype=np.uint8).reshape(-1, 32)
        return a

    def find_changes(self, hashes):
        """getChangeByHash for each hash: index of the applied change into the engine's list of changes, 0xffffffff where there is none."""
        a = self._hash_rows(hashes)
        out = np.full(a.shape[0], 0xFFFFFFFF, dtype=np.uint32)
        self._check(self._L.am355_find_changes(self._h, a.ctypes.data if a.size else None, a.shape[0], out.ctypes.data if a.size else None))
        return out

    def _index_query(self, fn, hashes):
        a = self._hash_rows(hashes)
        p, n = ctypes.c_void_p(), ctypes.c_uint32()
        self._check(fn(self._h, a.ctypes.data if a.size else None, a.shape[0], ctypes.byref(p), ctypes.byref(n)))
        return p, n.value

    def changes_since(self, have):
        """BackendDoc.getChanges(have) as indexes into the engine's list of changes, in the reference's order."""
        p, n = self._index_query(self._L.am355_changes_since, have)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)

    def changes_added(self, other):
        """BackendDoc(this).getChangesAdded(other) as indexes; `other`: the hashes of the changes the other state has applied."""
        p, n = self._index_query(self._L.am355_changes_added, other)
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)

    def missing_deps(self, heads=()):
        """BackendDoc.getMissingDeps(heads): sorted list of 32-byte hashes."""
        p, n = self._index_query(self._L.am355_missing_deps, heads)
        raw = ctypes.string_at(p, 32 * n) if n else b""
        return [raw[32 * k:32 * k + 32] for k in range(n)]

    def set_graph_probe_min(self, n):
        """Fewest membership probes of a hash-graph query that go to the device; 0xffffffff: never."""
        self._check(self._L.am355_set_graph_probe_min(self._h, int(n)))

    def graph_query_calls(self):
        """(membership tests of hash-graph queries answered on the device, by the host index)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_graph_query_calls(self._h, out))
        return int(out[0]), int(out[1])

    @staticmethod
    def _object_id(object_id):
        """"ctr@actorhex" (or "_root") as (counter, actor bytes, a ctypes buffer of them)."""
        if object_id == "_root":
            ctr, actor = 0, b""
        else:
            c, _, a = str(object_id).partition("@")
            if not c.isdigit() or not a or len(a) % 2:
                raise ValueError(f"not an object id: {object_id!r}")
            ctr, actor = int(c), bytes.fromhex(a)
        return ctr, actor, (ctypes.c_uint8 * max(len(actor), 1)).from_buffer_copy(actor or b"\0")

    def object_text(self, object_id):
        """The string of a Text object read on the device (am355_object_text): (utf-8 bytes, TextInfo). object_id: "ctr@actorhex" as in the
        patch. EngineError with code AM355_E_ARG: no such object / not a Text object."""
        ctr, actor, buf = self._object_id(object_id)
        p, n, info = ctypes.c_void_p(), ctypes.c_size_t(), TextInfo()
        self._check(self._L.am355_object_text(self._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(actor), ctypes.byref(p), ctypes.byref(n), ctypes.byref(info)))
        return (ctypes.string_at(p, n.value) if n.value else b""), info

    def object_text_calls(self):
        """(object_text calls served, kernel launches they made)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_object_text_calls(self._h, out))
        return int(out[0]), int(out[1])

    def text_limits(self):
        """(output bytes one gather workgroup owns, records per workgroup of the size pass, U+FEFF values looked at inline, walked at most)."""
        out = (ctypes.c_uint32 * 4)()
        self._check(self._L.am355_text_limits(out))
        return tuple(int(x) for x in out)

    def text_locate(self, object_id, first, n):
        """Elements [first, first + n) of a Text resolved to ids on the device (am355_text_locate): (runs, length). runs: a structured
        array (TEXT_RUN_DTYPE) of runs of consecutive (elemId, pred) pairs, actors as ranks; length: the Text's length. EngineError with
        code AM355_E_ARG: no such object / not a Text object / the range reaches past the length."""
        ctr, actor, buf = self._object_id(object_id)
        p, nr, length = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint64()
        self._check(self._L.am355_text_locate(self._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(actor), int(first), int(n), ctypes.byref(p), ctypes.byref(nr),
                                              ctypes.byref(length)))
        runs = np.zeros(nr.value, dtype=TEXT_RUN_DTYPE)
        if nr.value:
            ctypes.memmove(runs.ctypes.data, p, nr.value * TEXT_RUN_DTYPE.itemsize)
        return runs, int(length.value)

    def text_splice(self, object_id, start, deletions, values, actor, time=0, message=""):
        """One context.splice of the reference's frontend on a Text the engine holds (am355_text_splice): delete `deletions` elements from
        position `start` on, then insert the strings `values` there, one element each; `actor`: the author's id in hex. Returns the
        binary change (b"" when there was nothing to do); apply_patch_json() then gives the patch. EngineError with code AM355_E_ARG
        and the reference's RangeError text when the range is out of bounds, InvalidChanges with its TypeError text for a counter among
        the deleted elements. The caller owns the author and the order of its calls."""
        ctr, obj_actor, buf = self._object_id(object_id)
        parts = [v.encode("utf-8") for v in values]
        offs = np.zeros(len(parts) + 1, dtype=np.uint32)
        np.cumsum([len(b) for b in parts], out=offs[1:])
        blob = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8)
        author = np.frombuffer(bytes.fromhex(actor), dtype=np.uint8)
        msg = np.frombuffer(message.encode("utf-8") or b"\0", dtype=np.uint8)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.am355_text_splice(self._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(obj_actor), int(start), int(deletions), blob.ctypes.data,
                                              offs.ctypes.data, len(parts), author.ctypes.data if author.size else None, author.size, int(time), msg.ctypes.data,
                                              len(message.encode("utf-8")), ctypes.byref(p), ctypes.byref(n)))
        if n.value:
            self._n_changes = int(self.stats().n_changes)
        return ctypes.string_at(p, n.value) if n.value else b""

    def text_splice_calls(self):
        """(splices served, splices refused, kernel launches of the locate half of text_locate and text_splice)."""
        out = (ctypes.c_uint64 * 3)()
        self._check(self._L.am355_text_splice_calls(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def text_locate_limits(self):
        """(elements per workgroup of the locate kernel, elements the head scan takes in one workgroup, runs written straight to pinned memory)."""
        out = (ctypes.c_uint32 * 3)()
        self._check(self._L.am355_text_locate_limits(out))
        return tuple(int(x) for x in out)

    def list_locate(self, object_id, first, n):
        """Elements [first, first + n) of a plain list resolved to ids on the device (am355_list_locate): (runs, preds, length). runs: a
        structured array (LIST_RUN_DTYPE) of runs of consecutive elemIds, each with the range [pred_first, pred_first + pred_num) of
        preds (LIST_PRED_DTYPE; a run of several elements has one pred, which counts up with the elemId); actors as ranks. EngineError
        with code AM355_E_ARG: no such object / not a list object / the range reaches past the length."""
        ctr, actor, buf = self._object_id(object_id)
        p, q, nr, nq, length = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        self._check(self._L.am355_list_locate(self._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(actor), int(first), int(n), ctypes.byref(p), ctypes.byref(nr),
                                              ctypes.byref(q), ctypes.byref(nq), ctypes.byref(length)))
        runs, preds = np.zeros(nr.value, dtype=LIST_RUN_DTYPE), np.zeros(nq.value, dtype=LIST_PRED_DTYPE)
        if nr.value:
            ctypes.memmove(runs.ctypes.data, p, nr.value * LIST_RUN_DTYPE.itemsize)
        if nq.value:
            ctypes.memmove(preds.ctypes.data, q, nq.value * LIST_PRED_DTYPE.itemsize)
        return runs, preds, int(length.value)

    @staticmethod
    def _list_values(values):
        """values of list_splice / list_set as am355_local_value: a plain str / bool / None / int (-> int) / float (-> float64), or a
        pair (datatype, number) with datatype 'int', 'uint', 'float64', 'counter' or 'timestamp'."""
        out = np.zeros(len(values), dtype=_VALUE_DTYPE)
        strings = bytearray()
        for k, v in enumerate(values):
            datatype = None
            if isinstance(v, tuple):
                datatype, v = v
            if v is None and datatype is None:
                out[k]["tag"] = LV_NULL
            elif isinstance(v, bool) and datatype is None:
                out[k]["tag"] = LV_TRUE if v else LV_FALSE
            elif isinstance(v, str) and datatype is None:
                b = v.encode("utf-8")
                out[k] = (LV_UTF8, len(strings), len(b), 0, 0)
                strings.extend(b)
            elif isinstance(v, (bytes, bytearray)) and datatype is None:
                out[k]["tag"] = LV_BYTES
            elif isinstance(v, (int, float)) and not isinstance(v, bool):
                if datatype is None:
                    datatype = "int" if isinstance(v, int) else "float64"
                if datatype == "float64":
                    out[k] = (LV_FLOAT64, 0, 0, 0, int(np.array([float(v)], dtype="<f8").view("<u8")[0]))
                elif datatype in ("int", "uint", "counter", "timestamp") and isinstance(v, int) and abs(v) <= _MAX_SAFE and (datatype != "uint" or v >= 0):
                    out[k] = ({"counter": LV_COUNTER, "timestamp": LV_TIMESTAMP, "int": LV_INT, "uint": LV_UINT}[datatype], 0, 0, 0, v & 0xFFFFFFFFFFFFFFFF)
                else:
                    out[k]["tag"] = LV_BAD
            else:
                out[k]["tag"] = LV_BAD
        return out, np.frombuffer(bytes(strings) or b"\0", dtype=np.uint8), len(strings)

    def _list_call(self, call, object_id, where, values, actor, time, message):
        ctr, obj_actor, buf = self._object_id(object_id)
        vals, blob, blob_len = self._list_values(values)
        author = np.frombuffer(bytes.fromhex(actor), dtype=np.uint8)
        raw = message.encode("utf-8")
        msg = np.frombuffer(raw or b"\0", dtype=np.uint8)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        head = (self._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(obj_actor)) + where
        vargs = (vals.ctypes.data if vals.size else None, len(values)) if call == "splice" else (vals.ctypes.data,)
        fn = self._L.am355_list_splice if call == "splice" else self._L.am355_list_set
        self._check(fn(*head, *vargs, blob.ctypes.data, blob_len, author.ctypes.data if author.size else None, author.size, int(time), msg.ctypes.data, len(raw),
                       ctypes.byref(p), ctypes.byref(n)))
        if n.value:
            self._n_changes = int(self.stats().n_changes)
        return ctypes.string_at(p, n.value) if n.value else b""

    def list_splice(self, object_id, start, deletions, values, actor, time=0, message=""):
        """One context.splice of the reference's frontend on a plain list the engine holds (am355_list_splice): delete `deletions` elements
        from position `start` on, then insert `values` there (see _list_values for their form); `actor`: the author's id in hex. Returns
        the binary change (b"" when there was nothing to do); apply_patch_json() then gives the patch. EngineError with code AM355_E_ARG
        and the reference's RangeError text when the range is out of bounds, InvalidChanges with its TypeError text for a deleted element
        that shows a counter. The caller owns the author and the order of its calls."""
        return self._list_call("splice", object_id, (int(start), int(deletions)), list(values), actor, time, message)

    def list_set(self, object_id, index, value, actor, time=0, message=""):
        """list[index] = value (am355_list_set, context.js setListIndex): an index at or past the length inserts nulls up to it and the
        value; InvalidChanges with the reference's RangeError text onto an element that shows a counter. The op is always emitted: the
        reference skips an assignment of the value the element already shows, the engine holds no JS values to compare."""
        return self._list_call("set", object_id, (int(index),), [value], actor, time, message)

    def list_splice_calls(self):
        """(list_splice / list_set calls served, refused, kernel launches of the locate half of the three list calls)."""
        out = (ctypes.c_uint64 * 3)()
        self._check(self._L.am355_list_splice_calls(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def list_locate_limits(self):
        """(elements per workgroup of the locate kernel, elements the scan takes in one workgroup, runs / preds written straight to pinned memory)."""
        out = (ctypes.c_uint32 * 3)()
        self._check(self._L.am355_list_locate_limits(out))
        return tuple(int(x) for x in out)

    def map_locate(self, object_id, keys):
        """Keys (str, or UTF-8 bytes) of a map or table resolved on the device to the records of their visible values (am355_map_locate):
        (hits, recs). hits: MAP_HIT_DTYPE, one per key -- num values (0: absent) whose records are recs[first : first + num], in ascending
        op id; flags: MAP_COUNTER / MAP_CHILD of the value the map shows (the last record). recs: IR_MAP_DTYPE, actors as ranks.
        EngineError with code AM355_E_ARG: no such object / not a map object."""
        ctr, actor, buf = self._object_id(object_id)
        parts = [k.encode("utf-8") if isinstance(k, str) else bytes(k) for k in keys]
        offs = np.zeros(len(parts) + 1, dtype=np.uint32)
        np.cumsum([len(b) for b in parts], out=offs[1:])
        blob = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8)
        ph, pr, nr = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        self._check(self._L.am355_map_locate(self._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(actor), blob.ctypes.data, offs.ctypes.data, len(parts), ctypes.byref(ph),
                                             ctypes.byref(pr), ctypes.byref(nr)))
        hits, recs = np.zeros(len(parts), dtype=MAP_HIT_DTYPE), np.zeros(nr.value, dtype=IR_MAP_DTYPE)
        if len(parts):
            ctypes.memmove(hits.ctypes.data, ph, hits.nbytes)
        if nr.value:
            ctypes.memmove(recs.ctypes.data, pr, recs.nbytes)
        return hits, recs

    def map_get(self, object_id, keys):
        """What the keys of a map hold: {key: {opId: value}} with every visible value under its op id, as `props` of the reference's patch
        lists them ({} for an absent key). A primitive is {"value": v} (+ "datatype" for int / uint / float64 / counter / timestamp; a
        counter's value is its total), a child object {"objectId": its id}. Built from the records of map_locate and the host's arena."""
        keys = list(keys)
        hits, recs = self.map_locate(object_id, keys)
        a, o, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        self._check(self._L.am355_get_raw(self._h, ctypes.byref(a), ctypes.byref(o), ctypes.byref(n)))
        actors = {}
        out = {}
        for key, h in zip(keys, hits):
            held = {}
            for r in recs[int(h["first"]):int(h["first"]) + int(h["num"])]:
                rank = int(r["id_actor"])
                if rank not in actors:
                    actors[rank] = self.actor_of_rank(rank)
                op_id = f"{int(r['id_ctr'])}@{actors[rank]}"
                flags, tl = int(r["flags"]), int(r["val_tl"])
                if flags & MAP_CHILD:
                    held[op_id] = {"objectId": op_id}
                elif flags & MAP_COUNTER:
                    held[op_id] = {"value": int(r["counter"]), "datatype": "counter"}
                else:
                    raw = ctypes.string_at(a.value + int(r["val_off"]), tl >> 4) if tl >> 4 else b""
                    v, datatype = decode_ir_value(tl, raw)
                    held[op_id] = {"value": v} if datatype is None else {"value": v, "datatype": datatype}
            out[key] = held
        return out

    def map_update(self, object_id, ops, actor, time=0, message=""):
        """One change on one map the engine holds (am355_map_update): what Automerge.change(doc, d => { d.a = 1; delete d.b;
        d.n.increment(2) }) makes. ops: ("set", key, value) with value as for list_splice (see _list_values), ("del", key),
        ("inc", key, delta); `actor`: the author's id in hex. Returns the binary change (b"" when no op came of it: deletions of absent
        keys); apply_patch_json() then gives the patch. EngineError with code AM355_E_ARG and the reference's RangeError text for an empty
        key, InvalidChanges with its text for an assignment onto a counter (RangeError) and for an increment of what is no counter
        (TypeError). A set is always emitted: the engine holds no JS values to compare with."""
        ctr, obj_actor, buf = self._object_id(object_id)
        flat = np.zeros(len(ops), dtype=MAP_OP_DTYPE)
        strings, values = bytearray(), []
        for k, op in enumerate(ops):
            kind = {"set": MOP_SET, "del": MOP_DELETE, "inc": MOP_INC}[op[0]]
            key = op[1].encode("utf-8")
            flat[k] = (kind, len(strings), len(key), len(values) if kind == MOP_SET else 0, int(op[2]) if kind == MOP_INC else 0)
            strings.extend(key)
            if kind == MOP_SET:
                values.append(op[2])
        vals, vblob, vlen = self._list_values(values)
        vals["off"] += np.where(vals["tag"] == LV_UTF8, len(strings), 0).astype(np.uint32)   # (the values' strings stand behind the keys)
        blob = np.frombuffer(bytes(strings) + (vblob.tobytes()[:vlen]) or b"\0", dtype=np.uint8)
        author = np.frombuffer(bytes.fromhex(actor), dtype=np.uint8)
        raw = message.encode("utf-8")
        msg = np.frombuffer(raw or b"\0", dtype=np.uint8)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.am355_map_update(self._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(obj_actor), flat.ctypes.data if len(ops) else None, len(ops), blob.ctypes.data,
                                             len(strings) + vlen, vals.ctypes.data if vals.size else None, len(values), author.ctypes.data if author.size else None,
                                             author.size, int(time), msg.ctypes.data, len(raw), ctypes.byref(p), ctypes.byref(n)))
        if n.value:
            self._n_changes = int(self.stats().n_changes)
        return ctypes.string_at(p, n.value) if n.value else b""

    def map_calls(self):
        """(map_update calls served, refused, kernel launches of the locate half of map_locate and map_update)."""
        out = (ctypes.c_uint64 * 3)()
        self._check(self._L.am355_map_calls(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def map_locate_limits(self):
        """(records an object is searched through by the last round alone, keys read from pinned memory, hits / records written straight to
        pinned memory, G: the first gather has room for 2 n + G records)."""
        out = (ctypes.c_uint32 * 4)()
        self._check(self._L.am355_map_locate_limits(out))
        return tuple(int(x) for x in out)

    def set_map_locate_thread(self, on):
        """on: map_locate searches with one thread per key instead of one wavefront (measurement switch; same answers)."""
        self._check(self._L.am355_set_map_locate_thread(self._h, 1 if on else 0))

    def rank_of_actor(self, actor):
        """The rank of an actor (hex id) in the state's actor table (am355_rank_of_actor), None when the state does not know the actor.
        Ranks are renumbered when a new actor arrives: ask per call."""
        raw = bytes.fromhex(actor)
        buf = (ctypes.c_uint8 * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
        rank = ctypes.c_uint32()
        rc = self._L.am355_rank_of_actor(self._h, ctypes.cast(buf, ctypes.c_void_p), len(raw), ctypes.byref(rank))
        if rc == -2:   # AM355_E_ARG: no such actor
            return None
        self._check(rc)
        return int(rank.value)

    def actor_of_rank(self, rank):
        """The id (hex) of the actor with that rank (am355_actor_of_rank): the inverse of rank_of_actor."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._L.am355_actor_of_rank(self._h, int(rank), ctypes.byref(p), ctypes.byref(n)))
        return ctypes.string_at(p, n.value).hex()

    def text_positions(self, object_id, elem_ids):
        """ElemIds ("ctr@actorhex") of a Text resolved to positions on the device (am355_text_position): ([(status, position,
        is_counter)], length). status: POS_VISIBLE (position = the element's index), POS_DELETED (position = the visible elements in
        front of where it stood), POS_UNKNOWN (no applied change inserted such an element into this Text; position 0). The caret
        directly behind a known element is position + (status == POS_VISIBLE). Actors are translated to ranks here, per call."""
        ctr, actor, buf = self._object_id(object_id)
        q = np.zeros(len(elem_ids), dtype=ELEM_ID_DTYPE)
        ranks = {}
        for k, e in enumerate(elem_ids):
            c, _, a = str(e).partition("@")
            if not c.isdigit() or not a or len(a) % 2:
                raise ValueError(f"not an element id: {e!r}")
            if a not in ranks:
                ranks[a] = self.rank_of_actor(a)
            # (a counter beyond 32 bits names no row: asked as an unknown actor's)
            known = ranks[a] is not None and int(c) <= 0xFFFFFFFF
            q[k] = (int(c) if known else 0, ranks[a] if known else 0xFFFFFFFF)
        p, length = ctypes.c_void_p(), ctypes.c_uint64()
        self._check(self._L.am355_text_position(self._h, ctr, ctypes.cast(buf, ctypes.c_void_p), len(actor), q.ctypes.data if len(q) else None, len(q), ctypes.byref(p),
                                                ctypes.byref(length)))
        out = np.zeros(len(q), dtype=ELEM_POS_DTYPE)
        if len(q):
            ctypes.memmove(out.ctypes.data, p, len(q) * ELEM_POS_DTYPE.itemsize)
        return [(int(s) & 3, int(pos), bool(int(s) & POS_COUNTER)) for pos, s in zip(out["position"], out["status"])], int(length.value)

    def text_position_calls(self):
        """(text_positions calls served, kernel launches they made)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_text_position_calls(self._h, out))
        return int(out[0]), int(out[1])

    def text_position_limits(self):
        """(queries one workgroup of the resolve kernel takes, results written straight to pinned memory)."""
        out = (ctypes.c_uint32 * 2)()
        self._check(self._L.am355_text_position_limits(out))
        return tuple(int(x) for x in out)

    def set_text_pinned_max(self, n_bytes):
        """Strings of up to n_bytes are gathered straight into pinned memory by object_text (measurement switch; 0: never)."""
        self._check(self._L.am355_set_text_pinned_max(self._h, int(n_bytes)))

    def prim_hash_probe(self, table_hashes, queries):
        """am355_test_hash_probe: index into table_hashes of every query, 0xffffffff where it is not there (table and probes on the device)."""
        t, q = self._hash_rows(table_hashes), self._hash_rows(queries)
        out = np.full(q.shape[0], 0x55555555, dtype=np.uint32)
        self._check(self._L.am355_test_hash_probe(self._h, t.ctypes.data if t.size else None, t.shape[0], q.ctypes.data if q.size else None, q.shape[0],
                                                  out.ctypes.data if q.size else None))
        return out

    def apply_patch_json(self):
        """JSON.stringify of the patch the last apply_changes returned (the reference's incremental patch)."""
        p = ctypes.c_char_p()
        n = ctypes.c_size_t()
        self._check(self._L.am355_apply_patch_json(self._h, ctypes.byref(p), ctypes.byref(n)))
        return ctypes.string_at(p, n.value).decode("utf-8")

    def fetch_ir(self):
        """Patch IR + envelope from HBM into host memory owned by the context (what the JS host materialises the patch from)."""
        self._check(self._L.am355_fetch_ir(self._h, None))

    def patch_json(self):
        p = ctypes.c_char_p()
        n = ctypes.c_size_t()
        self._check(self._L.am355_patch_json(self._h, ctypes.byref(p), ctypes.byref(n)))
        return ctypes.string_at(p, n.value).decode("utf-8")

    def save(self, reencode=False):
        """Backend.save(state): the document as one binary chunk (op columns encoded on the GPU). A loaded document returns
        the bytes it came from, as the reference does; reencode=True re-encodes its op columns instead (diagnostic)."""
        p = ctypes.c_void_p()
        n = ctypes.c_size_t()
        self._check(self._L.am355_save(self._h, 1 if reencode else 0, ctypes.byref(p), ctypes.byref(n)))
        return ctypes.string_at(p, n.value)

    def applied(self):
        """Input indexes of the applied changes in application order (BackendDoc.changes / getAllChanges order)."""
        n = ctypes.c_uint32()
        self._check(self._L.am355_get_applied(self._h, None, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        self._check(self._L.am355_get_applied(self._h, out.ctypes.data if n.value else None, ctypes.byref(n)))
        return out

    def stats(self):
        s = Stats()
        self._check(self._L.am355_get_stats(self._h, ctypes.byref(s)))
        return s

    # ---- objectId sharding (one Engine per GPU / process) ---------------------------------------------------
    def set_shard(self, rank, world):
        self._check(self._L.am355_set_shard(self._h, rank, world))

    def fragment_size(self):
        n = ctypes.c_size_t()
        self._check(self._L.am355_fragment_size(self._h, ctypes.byref(n)))
        return n.value

    def export_fragment(self, ptr, capacity, device):
        """This rank's record tables into caller memory at `ptr` (device or host); returns the bytes written."""
        n = ctypes.c_size_t()
        self._check(self._L.am355_export_fragment(self._h, ctypes.c_void_p(ptr), capacity, 1 if device else 0, ctypes.byref(n)))
        return n.value

    def import_fragments(self, frags, offsets):
        """frags: uint8 host array holding the fragments of all ranks, offsets: uint64[world + 1]."""
        f = np.ascontiguousarray(frags, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(self._L.am355_import_fragments(self._h, f.ctypes.data, o.ctypes.data, o.size - 1))

    # ---- the same with the collective inside the library: RCCL over xGMI (am355_shard_init / am355_sharded_replay) ----
    def shard_unique_id(self):
        """128 bytes from ncclGetUniqueId (rank 0 makes them, the host carries them to the other ranks' processes)."""
        buf = (ctypes.c_uint8 * 128)()
        if self._L.am355_shard_unique_id(buf) != AM355_OK:
            raise EngineError(AM355_E_DEVICE, "RCCL is not available (librccl.so.1, or AM355_RCCL_LIB)")
        return bytes(buf)

    def shard_init(self, unique_id, rank, world):
        assert len(unique_id) == 128
        self._check(self._L.am355_shard_init(self._h, ctypes.c_char_p(bytes(unique_id)), rank, world))

    def sharded_replay(self, stitch_on_all_ranks=False):
        """am355_replay of the staged batch + ncclAllGather of the fragments + stitch (rank 0, or every rank)."""
        self._check(self._L.am355_sharded_replay(self._h, 1 if stitch_on_all_ranks else 0))

    def shard_fragment_bytes(self, world):
        out = np.zeros(world, dtype=np.uint64)
        self._check(self._L.am355_shard_fragment_bytes(self._h, out.ctypes.data, world))
        return out

    def shard_finalize(self):
        self._check(self._L.am355_shard_finalize(self._h))

    def resident_counters(self):
        """(calls of apply_changes that merged the batch alone into the resident state, calls that asked for it and took the full replay,
        calls of the first kind that also merged their new list elements into the stored order in place)."""
        out = (ctypes.c_uint64 * 3)()
        self._check(self._L.am355_resident_counters(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def resident_maps_only_calls(self):
        """Calls of apply_changes onto the resident state whose batch held plain map rows only (the map half of the merge ran alone)."""
        out = ctypes.c_uint64()
        self._check(self._L.am355_resident_maps_only_calls(self._h, ctypes.byref(out)))
        return int(out.value)

    def set_resident_new_actors(self, on):
        """on: a batch whose authors the document does not know yet is served on the resident state (the actors are inserted into the sorted
        table, one kernel renumbers the ranks the state holds) instead of by the full replay. Off by default."""
        self._check(self._L.am355_set_resident_new_actors(self._h, 1 if on else 0))

    def resident_new_actor_calls(self):
        """(calls served on the resident state that inserted at least one actor, those of them that launched the rank rewrite)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_resident_new_actor_calls(self._h, out))
        return int(out[0]), int(out[1])

    def set_resident_map_merge(self, on):
        """on: the plain map rows of a batch (`set` / `del` on string keys) are merged into the stored map records of the resident state
        instead of every record being emitted and ordered again; a document without a list is served that way too. Off by default."""
        self._check(self._L.am355_set_resident_map_merge(self._h, 1 if on else 0))

    def resident_map_merge_calls(self):
        """(resident calls whose map rows were merged into the stored map table in place, calls that tried, declined and were served by
        the path of before)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_resident_map_merge_calls(self._h, out))
        return int(out[0]), int(out[1])

    def set_resident_new_objects(self, on):
        """on: a batch that makes objects (`doc.cards.push({...})`, `doc.notes = new Text(...)`) is merged into the resident state in place
        -- the new objects take the next indexes of the stored object table and the end of the stored list order -- instead of every
        list being ranked and every table rebuilt by merge_run. Off by default."""
        self._check(self._L.am355_set_resident_new_objects(self._h, 1 if on else 0))

    def resident_new_object_calls(self):
        """(resident calls whose batch made at least one object and was served without merge_run, calls that tried, declined and went on
        with merge_run)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_resident_new_object_calls(self._h, out))
        return int(out[0]), int(out[1])

    def set_resident_counters(self, on):
        """on: the increments of map counters in a batch (`doc.votes.increment()`) are written into the stored map records in place --
        the rest of the batch is merged in place as before -- instead of the call running merge_run over the whole document. Off by
        default."""
        self._check(self._L.am355_set_resident_counters(self._h, 1 if on else 0))

    def resident_counter_calls(self):
        """(resident calls whose increments were written into the stored map records in place, with no merge_run and no map half; calls
        where the stage tried and declined, served by the map half)."""
        out = (ctypes.c_uint64 * 2)()
        self._check(self._L.am355_resident_counter_calls(self._h, out))
        return int(out[0]), int(out[1])

    def raw(self):
        """(arena, offsets) as staged: the uncompressed change containers back to back (copies)."""
        a, o, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        self._check(self._L.am355_get_raw(self._h, ctypes.byref(a), ctypes.byref(o), ctypes.byref(n)))
        offs = np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_uint64)), shape=(n.value + 1,)).copy()
        size = int(offs[-1])
        arena = np.ctypeslib.as_array(ctypes.cast(a, ctypes.POINTER(ctypes.c_uint8)), shape=(size,)).copy() if size else np.zeros(0, dtype=np.uint8)
        return arena, offs

    def doc_changes(self, deflate=True):
        """History of a loaded document: (arena, offsets, hashes) = the binary changes Backend.getAllChanges(Backend.load(doc)) returns,
        back to back in document order, and their 32-byte hashes (reference new.js:1887-1912, columnar.js:876-981). Copies."""
        a, o, n, h = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_void_p()
        self._check(self._L.am355_doc_changes(self._h, 1 if deflate else 0, ctypes.byref(a), ctypes.byref(o), ctypes.byref(n), ctypes.byref(h)))
        offs = np.ctypeslib.as_array(ctypes.cast(o, ctypes.POINTER(ctypes.c_uint64)), shape=(n.value + 1,)).copy()
        size = int(offs[-1])
        arena = np.ctypeslib.as_array(ctypes.cast(a, ctypes.POINTER(ctypes.c_uint8)), shape=(size,)).copy() if size else np.zeros(0, dtype=np.uint8)
        hashes = np.ctypeslib.as_array(ctypes.cast(h, ctypes.POINTER(ctypes.c_uint8)), shape=(n.value, 32)).copy() if n.value else np.zeros((0, 32), dtype=np.uint8)
        return arena, offs, hashes

    def hashes(self):
        out = np.zeros((self._n_changes, 32), dtype=np.uint8)
        self._check(self._L.am355_get_hashes(self._h, out.ctypes.data))
        return out

    # ---- diagnostics ------------------------------------------------------------------------------------
    def test_sort(self, keys, vals, key_bits=64):
        k = np.ascontiguousarray(keys, dtype=np.uint64).copy()
        v = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        self._check(self._L.am355_test_sort(self._h, k.ctypes.data, v.ctypes.data, k.size, key_bits))
        return k, v

    def test_scan(self, values):
        a = np.ascontiguousarray(values, dtype=np.uint32)
        out = np.zeros_like(a)
        total = np.zeros(1, dtype=np.uint32)
        self._check(self._L.am355_test_scan(self._h, a.ctypes.data, out.ctypes.data, a.size, total.ctypes.data))
        return out, int(total[0])

    # The primitives one by one (am355_test_* of include/am355.h). Buffers are images: copies go to the device whole and come back whole,
    # so the words around a range can be compared as well. `total` arguments: None = not asked for, else the word's value before the call.
    @staticmethod
    def _img(a, dtype=np.uint32):
        return None if a is None else np.ascontiguousarray(a, dtype=dtype).copy()

    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data

    def prim_scan(self, in_buf, in_off, n, out_buf=None, out_off=0, total=None):
        """exclusive_scan_u32 from in_buf[in_off:] into out_buf[out_off:] (None: in place). Returns (in_buf, out_buf, total) afterwards."""
        a, o = self._img(in_buf), self._img(out_buf)
        t = None if total is None else np.array([total], dtype=np.uint32)
        self._check(self._L.am355_test_scan_at(self._h, a.ctypes.data, a.size, in_off, self._ptr(o), 0 if o is None else o.size, in_off if o is None else out_off, n, self._ptr(t)))
        return a, o, None if t is None else int(t[0])

    def prim_scan2(self, in_a, in_b, in_off, n, out_a=None, out_b=None, out_off=0, total_a=None, total_b=None):
        a, b, oa, ob = self._img(in_a), self._img(in_b), self._img(out_a), self._img(out_b)
        ta = None if total_a is None else np.array([total_a], dtype=np.uint32)
        tb = None if total_b is None else np.array([total_b], dtype=np.uint32)
        self._check(self._L.am355_test_scan2(self._h, a.ctypes.data, b.ctypes.data, a.size, in_off, self._ptr(oa), self._ptr(ob), 0 if oa is None else oa.size,
                                             in_off if oa is None else out_off, n, self._ptr(ta), self._ptr(tb)))
        return a, b, oa, ob, None if ta is None else int(ta[0]), None if tb is None else int(tb[0])

    def prim_scan_terminators(self, bytes_buf, byte_off, L, out_buf, out_off, total=None):
        b, o = self._img(bytes_buf, np.uint8), self._img(out_buf)
        t = None if total is None else np.array([total], dtype=np.uint32)
        self._check(self._L.am355_test_scan_terminators(self._h, b.ctypes.data, b.size, byte_off, L, o.ctypes.data, o.size, out_off, self._ptr(t)))
        return o, None if t is None else int(t[0])

    def prim_max(self, values, before):
        v = self._img(values)
        t = np.array([before], dtype=np.uint32)
        self._check(self._L.am355_test_max(self._h, v.ctypes.data, v.size, t.ctypes.data))
        return int(t[0])

    def prim_sort(self, keys, vals, begin_bit, end_bit, first_table=None):
        """radix_sort_pairs. Returns (keys, vals, the buffer the sort said holds them)."""
        k, v, tab = self._img(keys, np.uint64), self._img(vals), self._img(first_table)
        res = ctypes.c_int(-1)
        self._check(self._L.am355_test_sort_bits(self._h, k.ctypes.data, v.ctypes.data, k.size, begin_bit, end_bit, self._ptr(tab), ctypes.byref(res)))
        return k, v, res.value

    def prim_chain_mark(self, nxt, mark, n):
        nx, m = self._img(nxt), self._img(mark)
        self._check(self._L.am355_test_chain_mark(self._h, nx.ctypes.data, m.ctypes.data, m.size, n))
        return m

    def prim_remap(self, buf, base_off, ranges, table):
        """ranges: [(first word, count, stride, guard, guard_skip)]. Returns (buf, ranges the table held)."""
        b, tab = self._img(buf), self._img(table)
        r = np.array([[f, c, s, g & 0xFFFFFFFF, k] for f, c, s, g, k in ranges], dtype=np.uint32).reshape(-1, 5)
        added = ctypes.c_uint32(0)
        self._check(self._L.am355_test_remap(self._h, b.ctypes.data, b.size, base_off, r.ctypes.data, len(ranges), tab.ctypes.data, tab.size, ctypes.byref(added)))
        return b, added.value

    def prim_fill(self, buf, base_off, ranges):
        """ranges: [(first word, bytes, value)]."""
        b = self._img(buf)
        r = np.array(ranges, dtype=np.uint32).reshape(-1, 3)
        added = ctypes.c_uint32(0)
        self._check(self._L.am355_test_fill(self._h, b.ctypes.data, b.size, base_off, r.ctypes.data, len(ranges), ctypes.byref(added)))
        return b, added.value

    def prim_copy(self, dst, src, ranges, src_pinned):
        """ranges: [(dst byte offset, src byte offset, bytes)]."""
        d, s = self._img(dst, np.uint8), self._img(src, np.uint8)
        r = np.array(ranges, dtype=np.uint32).reshape(-1, 3)
        added = ctypes.c_uint32(0)
        self._check(self._L.am355_test_copy(self._h, d.ctypes.data, d.size, s.ctypes.data, s.size, 1 if src_pinned else 0, r.ctypes.data, len(ranges), ctypes.byref(added)))
        return d, added.value

    def prim_signal_words(self, a, b, seq, host_words, seq_word):
        wa, wb, h = self._img(a), self._img(b), self._img(host_words)
        s = np.array([seq_word], dtype=np.uint32)
        self._check(self._L.am355_test_signal_words(self._h, wa.ctypes.data, wa.size, wb.ctypes.data, wb.size, seq, h.ctypes.data, h.size, s.ctypes.data))
        return h, int(s[0])

    def prim_carried_scan(self, values):
        """Returns (carry_prefix over the grid, block_exclusive_scan_u32 within each workgroup, the workgroups' sums)."""
        v = self._img(values)
        out, out_wg, tot = np.empty_like(v), np.empty_like(v), np.empty((v.size + 255) // 256, dtype=np.uint32)
        self._check(self._L.am355_test_carried_scan(self._h, v.ctypes.data, v.size, out.ctypes.data, out_wg.ctypes.data, tot.ctypes.data))
        return out, out_wg, tot

    def prim_text_premises(self, table, begin, n_recs, n_values, length_before=0xdeadbeef):
        """am355_test_text_premises: the check pass of the Text calls over records [begin, begin + n_recs) of `table` (IR_EDIT_DTYPE, the
        sentinel among its records). Returns (flag word, length word behind the pass)."""
        t = np.ascontiguousarray(table, dtype=IR_EDIT_DTYPE)
        flags, length = ctypes.c_uint32(0), ctypes.c_uint32(length_before)
        self._check(self._L.am355_test_text_premises(self._h, t.ctypes.data, t.size, begin, n_recs, n_values, ctypes.byref(flags), ctypes.byref(length)))
        return flags.value, length.value

    def prim_list_premises(self, table, begin, n_recs, n_values, length_before=0xdeadbeef):
        """am355_test_list_premises: the same over the check pass of the calls on a plain list (bit 8: an element without an insert)."""
        t = np.ascontiguousarray(table, dtype=IR_EDIT_DTYPE)
        flags, length = ctypes.c_uint32(0), ctypes.c_uint32(length_before)
        self._check(self._L.am355_test_list_premises(self._h, t.ctypes.data, t.size, begin, n_recs, n_values, ctypes.byref(flags), ctypes.byref(length)))
        return flags.value, length.value

    def rows(self):
        n = int(self.stats().n_ops)
        names = ["obj_actor", "obj_ctr", "key_actor", "key_ctr", "key_off", "key_len", "action", "val_tl", "val_off", "pred_num",
                 "id_ctr", "id_actor", "insert", "succ_cnt"]
        arrs = {k: np.zeros(n, dtype=np.uint8 if k == "insert" else np.uint32) for k in names}
        self._check(self._L.am355_get_rows(self._h, *[arrs[k].ctypes.data for k in names]))
        return arrs


def replay_patch_json(log, device=0, lib_path=DEFAULT_LIB):
    """Backend.getPatch(Backend.loadChanges(Backend.init(), changes)) as JSON text, computed on the GPU."""
    eng = Engine(device, lib_path)
    try:
        eng.load_changes(log)
        eng.replay()
        return eng.patch_json()
    finally:
        eng.close()
