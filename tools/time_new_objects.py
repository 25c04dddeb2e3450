"""What a change that MAKES objects costs am355_apply_changes on a large kept state (host to host: each call ends with the incremental
patch assembled on the host), with am355_set_resident_new_objects and without.

The state: loggen.config("c4_text_single", scale) -- ~1 M op rows at scale 1.0 -- and, from a second, independent log by one more
author, a root list of 1,000 cards ({title, done}). No generator kind of loggen makes objects inside a session, so that log is made
here: CardsLog below writes its changes in the reference's change format (columnar.js:635-760; its own encoder, nothing shared
with the engine). Calls timed, all by the cards' author:
    (a) one change pushing one card                      (16 calls)
    (b) 40 such changes in one call                      (4 calls)
    (c) one change making a Text on a root key and typing 200 characters into it   (8 calls)

    python tools/time_new_objects.py [--lib libam355.so] [--scale 1.0] [--label text] [--off] [--check]

--lib: another build of the engine (the parent commit's, for the A/B): a library without am355_set_resident_new_objects serves these
calls by merge_run. --off: this library with the switch left off. --check: every call's patch against the sequential oracle (small
scales: the oracle replays on one thread). Prints the per-call times, their median and max, and the path counters."""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from automerge_classic_amd import engine, loggen  # noqa: E402
from automerge_classic_amd.loggen import ChangeLog  # noqa: E402


# ---- the change format, as far as these changes need it ----
def uleb(v):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def sleb(v):
    out = bytearray()
    while True:
        b = v & 0x7f
        v >>= 7
        if (v == 0 and not b & 0x40) or (v == -1 and b & 0x40):
            out.append(b)
            return bytes(out)
        out.append(b | 0x80)


def rle(values, enc):
    """Run-length column (encoding.js RLEEncoder): a run of equal values as (count, value), lone values gathered into (-n, values),
    nulls as (0, count); a column of nulls only is empty."""
    if all(v is None for v in values):
        return b""
    runs = []
    for v in values:
        if runs and runs[-1][0] == v:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    out, lone = bytearray(), []

    def flush():
        if lone:
            out.extend(sleb(-len(lone)))
            for x in lone:
                out.extend(enc(x))
            lone.clear()
    for v, n in runs:
        if v is None:
            flush()
            out.extend(sleb(0) + uleb(n))
        elif n == 1:
            lone.append(v)
        else:
            flush()
            out.extend(sleb(n) + enc(v))
    flush()
    return bytes(out)


def delta(values):
    out, last = [], 0
    for v in values:
        if v is None:
            out.append(None)
        else:
            out.append(v - last)
            last = v
    return rle(out, sleb)


def booleans(values):
    out, cur, n = bytearray(), False, 0
    for v in values:
        if v == cur:
            n += 1
        else:
            out.extend(uleb(n))
            cur, n = v, 1
    if n:
        out.extend(uleb(n))
    return bytes(out)


def utf8(s):
    b = s.encode()
    return uleb(len(b)) + b


MAKE_MAP, SET, MAKE_LIST, MAKE_TEXT = 0, 1, 2, 4
HEAD = (None, 0)   # elemId '_head'


class CardsLog:
    """One author's log: a root list `cards` of {title, done} maps, Texts on root keys. Ops: dicts with obj (None: _root, else the make
    op's counter), key (a string, or (actor, counter) of the reference element for a list op), insert, action, value (None, a bool or
    a string). Every id is the author's own: actor index 0 wherever a column asks for one."""

    def __init__(self, actor_hex):
        self.actor = bytes.fromhex(actor_hex)
        self.seq, self.op, self.dep = 0, 0, None
        self.cards_obj, self.last_card, self.n_cards, self.n_texts = None, None, 0, 0

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
            elif isinstance(v, bool):
                val_len.append(2 if v else 1)
            else:
                b = v.encode()
                val_len.append(len(b) << 4 | 6)
                val_raw.extend(b)
        cols = [(1, rle(obj_actor, uleb)), (2, rle(obj_ctr, uleb)), (17, rle(key_actor, uleb)), (19, delta(key_ctr)), (21, rle(key_str, utf8)),
                (52, booleans([o["insert"] for o in ops])), (66, rle([o["action"] for o in ops], uleb)), (86, rle(val_len, uleb)), (87, bytes(val_raw)),
                (112, rle([0] * len(ops), uleb))]
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
        self.cards_obj = self.op + 1
        return self.change([dict(obj=None, key="cards", insert=False, action=MAKE_LIST, value=None)])

    def push_cards(self, n):
        ops = []
        for _ in range(n):
            card = self.op + len(ops) + 1
            ops.append(dict(obj=self.cards_obj, key=HEAD if self.last_card is None else (0, self.last_card), insert=True, action=MAKE_MAP, value=None))
            ops.append(dict(obj=card, key="title", insert=False, action=SET, value="card %d" % self.n_cards))
            ops.append(dict(obj=card, key="done", insert=False, action=SET, value=self.n_cards % 2 == 0))
            self.last_card = card
            self.n_cards += 1
        return self.change(ops)

    def text_with(self, n_chars):
        text = self.op + 1
        ops = [dict(obj=None, key="notes%d" % self.n_texts, insert=False, action=MAKE_TEXT, value=None)]
        for k in range(n_chars):
            ops.append(dict(obj=text, key=HEAD if k == 0 else (0, text + k), insert=True, action=SET, value="abcdefghij"[k % 10]))
        self.n_texts += 1
        return self.change(ops)


def changes_of(log):
    arena, offs = bytes(log.arena), [int(x) for x in log.offsets]
    return [arena[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--label", default="")
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()

    cards = CardsLog("c0" * 16)
    head = changes_of(loggen.config("c4_text_single", args.scale)) + [cards.setup()] + [cards.push_cards(100) for _ in range(10)]
    eng = engine.Engine(0, args.lib) if args.lib else engine.Engine(0)
    has = hasattr(eng._L, "am355_set_resident_new_objects")
    on = has and not args.off
    if on:
        eng.set_resident_new_objects(True)
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
        call([cards.push_cards(1)])
    call([cards.text_with(200)])
    one = [call([cards.push_cards(1)]) for _ in range(16)]
    forty = [call([cards.push_cards(1) for _ in range(40)]) for _ in range(4)]
    text = [call([cards.text_with(200)]) for _ in range(8)]

    def line(what, ms):
        s = sorted(ms)
        return "%-34s median %.3f ms  max %.3f ms  min %.3f ms   [%s]" % (what, (s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2, s[-1], s[0], " ".join("%.3f" % t for t in ms))

    print("time_new_objects%s: c4_text_single scale %g + 1,000 cards, %d rows kept; switch %s%s" % (
        " (" + args.label + ")" if args.label else "", args.scale, rows, "on" if on else "off" if has else "absent (merge_run for make-calls)",
        "; every patch checked against the oracle" if session is not None else ""))
    print(line("(a) one change pushing one card", one))
    print(line("(b) 40 such changes in one call", forty))
    print(line("(c) makeText + 200 characters", text))
    print("resident counters (served, fell back, in place):", eng.resident_counters(), " map-half calls:", eng.resident_maps_only_calls(),
          " new-object calls (in place, declined):", eng.resident_new_object_calls() if has else "n/a")
    if session is not None:
        session.close()
    eng.close()


if __name__ == "__main__":
    main()
