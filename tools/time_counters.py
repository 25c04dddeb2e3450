"""What a counter increment costs am355_apply_changes on a large kept state (host to host: each call ends with the incremental patch
assembled on the host), with am355_set_resident_counters and without.

The state: loggen.config("c4_text_single", scale) -- ~1 M op rows at scale 1.0 -- and, from a second, independent log by one more
author, a root map of 1,000 keys, 100 of them counters, and a Text of that author's. No generator kind of loggen increments a counter
inside a session, so that log is made here: CounterLog below writes its changes in the reference's change format (columnar.js:635-760;
the column encoders are tools/time_new_objects.py's, nothing shared with the engine). Calls timed, all by that author:
    (a) one change with one increment                                  (16 calls)
    (b) 40 such changes in one call                                    (4 calls)
    (c) one change that types 200 characters and increments once       (8 calls)

    python tools/time_counters.py [--lib libam355.so] [--scale 1.0] [--label text] [--off] [--check]

--lib: another build of the engine (the parent commit's, for the A/B): a library without am355_set_resident_counters serves these calls
by merge_run. --off: this library with the switch left off. --check: every call's patch against the sequential oracle (small scales:
the oracle replays on one thread). Prints the per-call times, their median and max, and the path counters."""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from automerge_classic_amd import engine, loggen  # noqa: E402
from automerge_classic_amd.loggen import ChangeLog  # noqa: E402
from time_new_objects import HEAD, booleans, changes_of, delta, rle, sleb, uleb, utf8  # noqa: E402

SET, MAKE_TEXT, INC = 1, 4, 5
N_KEYS, N_COUNTERS = 1000, 100


class CounterLog:
    """One author's log: a root map of plain keys and counters, a Text on a root key. Ops: dicts with obj (None: _root, else the make
    op's counter), key (a string, or (actor, counter) of the reference element for a list op), insert, action, value (None, a string,
    ("int", v) or ("counter", v)) and pred (None, or the counter of the op it succeeds). Every id is the author's own: actor index 0
    wherever a column asks for one."""

    def __init__(self, actor_hex):
        self.actor = bytes.fromhex(actor_hex)
        self.seq, self.op, self.dep = 0, 0, None
        self.counter_op = {}   # key -> the op that set the counter
        self.text, self.last_char, self.n_incs = None, None, 0

    def change(self, ops):
        self.seq += 1
        start = self.op + 1
        self.op += len(ops)
        obj_actor = [None if o["obj"] is None else 0 for o in ops]
        obj_ctr = [o["obj"] for o in ops]
        elem = [o["key"] if isinstance(o["key"], tuple) else None for o in ops]
        key_actor = [None if e is None or e == HEAD else 0 for e in elem]
        key_ctr = [None if e is None else e[1] for e in elem]
        key_str = [o["key"] if isinstance(o["key"], str) else None for o in ops]
        val_len, val_raw = [], bytearray()
        for o in ops:
            v = o["value"]
            if v is None:
                val_len.append(0)
            elif isinstance(v, str):
                b = v.encode()
                val_len.append(len(b) << 4 | 6)
                val_raw.extend(b)
            else:
                b = sleb(v[1])
                val_len.append(len(b) << 4 | (8 if v[0] == "counter" else 4))
                val_raw.extend(b)
        preds = [o["pred"] for o in ops if o.get("pred") is not None]
        cols = [(1, rle(obj_actor, uleb)), (2, rle(obj_ctr, uleb)), (17, rle(key_actor, uleb)), (19, delta(key_ctr)), (21, rle(key_str, utf8)),
                (52, booleans([o["insert"] for o in ops])), (66, rle([o["action"] for o in ops], uleb)), (86, rle(val_len, uleb)), (87, bytes(val_raw)),
                (112, rle([0 if o.get("pred") is None else 1 for o in ops], uleb)), (113, rle([0] * len(preds), uleb)), (115, delta(preds))]
        cols = [(cid, buf) for cid, buf in cols if buf]
        body = bytearray()
        body.extend(uleb(0 if self.dep is None else 1))
        if self.dep is not None:
            body.extend(self.dep)
        body.extend(uleb(len(self.actor)) + self.actor + uleb(self.seq) + uleb(start) + sleb(0) + uleb(0) + uleb(0))
        body.extend(uleb(len(cols)))
        for cid, buf in cols:
            body.extend(uleb(cid) + uleb(len(buf)))
        for _, buf in cols:
            body.extend(buf)
        chunk = b"\x01" + uleb(len(body)) + bytes(body)
        self.dep = hashlib.sha256(chunk).digest()
        return b"\x85\x6f\x4a\x83" + self.dep[:4] + chunk

    def setup(self):
        """N_KEYS root keys in one change, every tenth a counter; a Text `notes` with one character."""
        ops = []
        for k in range(N_KEYS):
            key = "key%04d" % k
            if k % (N_KEYS // N_COUNTERS) == 0:
                self.counter_op[key] = self.op + len(ops) + 1
                ops.append(dict(obj=None, key=key, insert=False, action=SET, value=("counter", k)))
            else:
                ops.append(dict(obj=None, key=key, insert=False, action=SET, value="value %d" % k))
        self.text = self.op + len(ops) + 1
        ops.append(dict(obj=None, key="notes", insert=False, action=MAKE_TEXT, value=None))
        ops.append(dict(obj=self.text, key=HEAD, insert=True, action=SET, value="n"))
        self.last_char = self.text + 1
        return self.change(ops)

    def inc_op(self):
        keys = sorted(self.counter_op)
        key = keys[(self.n_incs * 37) % len(keys)]   # (a different counter every time, all over the key range)
        self.n_incs += 1
        return dict(obj=None, key=key, insert=False, action=INC, value=("int", 1 + self.n_incs % 5), pred=self.counter_op[key])

    def increment(self):
        return self.change([self.inc_op()])

    def type_and_increment(self, n_chars):
        ops = []
        for k in range(n_chars):
            ops.append(dict(obj=self.text, key=(0, self.last_char), insert=True, action=SET, value="abcdefghij"[k % 10]))
            self.last_char = self.op + len(ops)
        ops.append(self.inc_op())
        return self.change(ops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--label", default="")
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()

    author = CounterLog("c0" * 16)
    head = changes_of(loggen.config("c4_text_single", args.scale)) + [author.setup()]
    eng = engine.Engine(0, args.lib) if args.lib else engine.Engine(0)
    has = hasattr(eng._L, "am355_set_resident_counters")
    on = has and not args.off
    if on:
        eng.set_resident_counters(True)
    session = None
    if args.check:
        import json
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib
        session = oracle_lib.OracleSession()

    def call(batch):
        log = ChangeLog.from_changes(batch)
        t0 = time.perf_counter()
        eng.apply_changes(log)   # (returns with the incremental patch assembled on the host: behind every device wait of the call)
        ms = (time.perf_counter() - t0) * 1e3
        if session is not None:
            assert json.loads(eng.apply_patch_json()) == json.loads(session.apply(batch)), "the patch differs from the oracle's"
        return ms

    call(head)
    rows = int(eng.stats().n_ops)
    for _ in range(4):   # (warm: the path, its buffers)
        call([author.increment()])
    call([author.type_and_increment(200)])
    one = [call([author.increment()]) for _ in range(16)]
    forty = [call([author.increment() for _ in range(40)]) for _ in range(4)]
    typed = [call([author.type_and_increment(200)]) for _ in range(8)]

    def line(what, ms):
        s = sorted(ms)
        return "%-36s median %.3f ms  max %.3f ms  min %.3f ms   [%s]" % (what, (s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, s[-1], s[0], " ".join("%.3f" % t for t in ms))

    print("time_counters%s: c4_text_single scale %g + %d root keys, %d of them counters, %d rows kept; switch %s%s" % (
        " (" + args.label + ")" if args.label else "", args.scale, N_KEYS, N_COUNTERS, rows, "on" if on else "off" if has else "absent (merge_run for increment calls)",
        "; every patch checked against the oracle" if session is not None else ""))
    print(line("(a) one change with one increment", one))
    print(line("(b) 40 such changes in one call", forty))
    print(line("(c) 200 characters + one increment", typed))
    print("resident counters (served, fell back, in place):", eng.resident_counters(), " map-half calls:", eng.resident_maps_only_calls(),
          " counter calls (in place, declined):", eng.resident_counter_calls() if has else "n/a")
    if session is not None:
        if has and on:
            assert eng.resident_counter_calls() == (4 + 1 + 16 + 4 + 8, 0), eng.resident_counter_calls()
        session.close()
    eng.close()


if __name__ == "__main__":
    main()
