"""Seeded random Kleenex programs and inputs (test support)."""
import random

ALPHA = "abc"


def _regex(r, depth):
    k = r.random()
    if depth <= 0 or k < 0.30:
        c = r.random()
        if c < 0.5:
            return r.choice(ALPHA)
        if c < 0.7:
            return "[%s]" % "".join(sorted(set(r.choice(ALPHA) for _ in range(2))))
        if c < 0.8:
            return "[^%s]" % r.choice(ALPHA)
        return "."
    if k < 0.50:
        return "%s%s" % (_regex(r, depth - 1), _regex(r, depth - 1))
    if k < 0.65:
        return "(%s|%s)" % (_regex(r, depth - 1), _regex(r, depth - 1))
    if k < 0.80:
        return "(%s)%s" % (_regex(r, depth - 1), r.choice(["*", "+", "?", "*?", "??"]))
    if k < 0.90:
        lo = r.randint(0, 2)
        return "(%s){%d,%d}" % (_regex(r, depth - 1), lo, lo + r.randint(0, 2))
    return "(%s){%d}" % (_regex(r, depth - 1), r.randint(1, 3))


def _term(r, depth):
    k = r.random()
    if depth <= 0 or k < 0.35:
        c = r.random()
        if c < 0.45:
            return "/%s/" % _regex(r, 2)
        if c < 0.65:
            return "~/%s/" % _regex(r, 2)
        if c < 0.95:
            return '"%s"' % "".join(r.choice("XYZ,") for _ in range(r.randint(1, 3)))
        return "1"
    if k < 0.60:
        return "%s %s" % (_term(r, depth - 1), _term(r, depth - 1))
    if k < 0.80:
        return "(%s | %s)" % (_term(r, depth - 1), _term(r, depth - 1))
    if k < 0.92:
        return "(%s)%s" % (_term(r, depth - 1), r.choice(["*", "+", "?"]))
    return "(%s){%d,%d}" % (_term(r, depth - 1), r.randint(0, 1), r.randint(1, 3))


def program(seed):
    r = random.Random(seed)
    body = _term(r, 3)
    if r.random() < 0.5:
        return "main := (%s)*\n" % body
    if r.random() < 0.5:
        return "main := (part /\\n/)*\npart := %s\n" % body
    return "main := %s\n" % body


def inputs(seed, count, maxlen):
    r = random.Random(seed * 7919 + 1)
    out = []
    for _ in range(count):
        n = r.randint(0, maxlen)
        out.append("".join(r.choice(ALPHA + "\n") if r.random() < 0.9 else r.choice("abcx") for _ in range(n)).encode())
    return out


# ------------------------------------------------------------------------------------------ accepted and rejected inputs
# A random string is almost never a long accepted input of a random grammar.  A program accepts an input exactly when some path
# through its nondeterministic transducer (host.dump_fst: init, final, eps, sym) does: a random walk over that transducer which
# never leaves the states from which a final state can be reached writes down an accepted input of any length the grammar has.
GROWTH_CAP = 40


class _Walk:
    """What the walk needs to know of one transducer: the edges as the lock-step simulator takes them (a state with ε-edges leaves
    through them only, and the run ends in a final state without any), per state the shortest way to such a final state as
    (symbols, edges) — None where there is none — and how many symbols a path from it can still consume, capped at GROWTH_CAP."""

    def __init__(self, fst):
        import heapq
        eps, sym = fst["eps"], fst["sym"]
        n = len(sym)
        self.init = fst["init"]
        self.inside = {}                        # (alphabet, ranges) -> the alphabet's bytes inside the ranges
        self.succ = [[(0, t, None) for _, t in eps[q]] if eps[q] else [(1, e[2], tuple(map(tuple, e[0]))) for e in sym[q]] for q in range(n)]
        pred = [[] for _ in range(n)]
        for q in range(n):
            for w, t, _ in self.succ[q]:
                pred[t].append((w, q))
        self.rank = [None] * n
        heap = [((0, 0), q) for q in set(fst["final"]) if not eps[q]]
        while heap:
            d, q = heapq.heappop(heap)
            if self.rank[q] is not None:
                continue
            self.rank[q] = d
            for w, s in pred[q]:
                if self.rank[s] is None:
                    heapq.heappush(heap, ((d[0] + w, d[1] + 1), s))
        self.grow = [0] * n
        todo = [q for q in range(n) if self.rank[q] is not None]
        while todo:
            t = todo.pop()
            for w, s in pred[t]:
                if self.rank[s] is not None and self.grow[s] < min(GROWTH_CAP, w + self.grow[t]):
                    self.grow[s] = min(GROWTH_CAP, w + self.grow[t])
                    todo.append(s)


def _byte_of(w, ranges, rnd, alphabet):
    if rnd.random() < 0.9:
        inside = w.inside.get((alphabet, ranges))
        if inside is None:
            inside = w.inside[(alphabet, ranges)] = [b for b in alphabet if any(lo <= b <= hi for lo, hi in ranges)]
        if inside:
            return rnd.choice(inside)
    k = rnd.randrange(sum(hi - lo + 1 for lo, hi in ranges))
    for lo, hi in ranges:
        if k <= hi - lo:
            return lo + k
        k -= hi - lo + 1


def accepted_input(fst, rnd, length, alphabet=b"abc\n"):
    """An input that the transducer accepts, of `length` bytes and the few more that the nearest final state is away — or, where the
    grammar is bounded, the longest one this walk reached.  While bytes are wanted the walk prefers successors from which
    min(bytes wanted, GROWTH_CAP) more symbols can be consumed.  (The analysis is kept in the transducer's own dict.)"""
    w = fst.get("_walk")
    if w is None:
        w = fst["_walk"] = _Walk(fst)
    q = w.init
    if w.rank[q] is None:
        raise ValueError("the transducer accepts no input")
    out = bytearray()
    seen = set()                                # ε-targets since the last symbol: among equally good ways, not round an ε-loop again
    while len(out) < length and w.grow[q]:
        need = min(length - len(out), GROWTH_CAP)
        cands = [c for c in w.succ[q] if w.rank[c[1]] is not None]
        good = [c for c in cands if c[0] + w.grow[c[1]] >= need]
        if not good:
            best = max(c[0] + w.grow[c[1]] for c in cands)
            good = [c for c in cands if c[0] + w.grow[c[1]] == best]
        good = [c for c in good if c[0] or c[1] not in seen] or good
        step, q, ranges = rnd.choice(good)
        if step:
            out.append(_byte_of(w, ranges, rnd, alphabet))
            seen.clear()
        else:
            seen.add(q)
    while w.rank[q] != (0, 0):
        step, q, ranges = next(c for c in w.succ[q] if w.rank[c[1]] is not None and (w.rank[c[1]][0] + c[0], w.rank[c[1]][1] + 1) == w.rank[q])
        if step:
            out.append(_byte_of(w, ranges, rnd, alphabet))
    return bytes(out)


EDGE_POSITIONS = (63, 64, 4095, 4096)      # the last byte of a piece and of a wave-iteration, and the first of the next


def rejected_variants(data, rnd):
    """Inputs that differ from an accepted one in one place — one byte overwritten with x or FF, and the input cut there — at the edge
    positions, at the last byte and at a random one: a random string dies in its first symbols, these die where the walk was.
    (A variant may still be accepted: the caller asks the oracle.)"""
    if not data:
        return []
    at = sorted({p for p in EDGE_POSITIONS + (len(data) - 1, rnd.randrange(len(data))) if p < len(data)})
    out = []
    for p in at:
        out.append(data[:p] + rnd.choice((b"x", b"\xff")) + data[p + 1:])
        out.append(data[:p])
    return out


# ------------------------------------------------------------------------------------------------------- wider programs
WIDE = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMN"


def _wconst(r):
    """a constant of 1 byte (stored inline), of 2 to 16 bytes, or of 17 to 40 (beyond the 16-byte store sequence); some hold
    bytes >= 0x80 (a \\xNN of a string constant is that code point in UTF-8: two bytes)"""
    k = r.random()
    n = 1 if k < 0.3 else r.randint(2, 16) if k < 0.75 else r.randint(17, 40)
    out = []
    while n > 0:
        if n >= 2 and r.random() < 0.1:
            out.append(r.choice(["\\xe9", "\\xff", "\\x80"]))
            n -= 2
        else:
            out.append(r.choice("XYZ,;=<>"))
            n -= 1
    return '"%s"' % "".join(out)


def _wregex(r, depth):
    k = r.random()
    if depth <= 0 or k < 0.35:
        c = r.random()
        if c < 0.40:
            return r.choice(WIDE)
        if c < 0.55:
            return "[%s]" % "".join(sorted(set(r.choice(WIDE) for _ in range(r.randint(2, 5)))))
        if c < 0.65:
            lo = r.randrange(len(WIDE) - 1)
            return "[%s-%s]" % (WIDE[lo], WIDE[r.randrange(lo, min(lo + 12, 26 if lo < 26 else len(WIDE)))])
        if c < 0.75:
            return r.choice(["[\\xff]", "[\\x80-\\xff]", "[\\xa9\\xfe]", "[\\x80-\\xbf]", "[a\\xff]", "\\xe9"])
        if c < 0.85:
            return "[^%s]" % r.choice(list(WIDE[:6]) + ["\\xff", "\\n"])
        return "."
    if k < 0.55:
        return "%s%s" % (_wregex(r, depth - 1), _wregex(r, depth - 1))
    if k < 0.70:
        return "(%s|%s)" % (_wregex(r, depth - 1), _wregex(r, depth - 1))
    if k < 0.88:
        return "(%s)%s" % (_wregex(r, depth - 1), r.choice(["*", "+", "?", "*?", "??"]))
    lo = r.randint(0, 2)
    return "(%s){%d,%d}" % (_wregex(r, depth - 1), lo, lo + r.randint(0, 2))


def _wterm(r, depth):
    k = r.random()
    if depth <= 0 or k < 0.35:
        c = r.random()
        if c < 0.45:
            return "/%s/" % _wregex(r, 2)
        if c < 0.65:
            return "~/%s/" % _wregex(r, 2)
        if c < 0.95:
            return _wconst(r)
        return "1"
    if k < 0.60:
        return "%s %s" % (_wterm(r, depth - 1), _wterm(r, depth - 1))
    if k < 0.80:
        return "(%s | %s)" % (_wterm(r, depth - 1), _wterm(r, depth - 1))
    if k < 0.92:
        return "(%s)%s" % (_wterm(r, depth - 1), r.choice(["*", "+", "?"]))
    return "(%s){%d,%d}" % (_wterm(r, depth - 1), r.randint(0, 1), r.randint(1, 3))


def _letter_table(r):
    """every letter an alternative of its own, each with another replacement: as many byte classes as letters (more than the 31 whose
    class * 8 fits the class table's byte: the class table then holds indices)"""
    letters = WIDE[:r.randint(33, len(WIDE))]
    alts = []
    for c in letters:
        k = r.random()
        alts.append("~/%s/ %s" % (c, _wconst(r)) if k < 0.6 else "/%s/ %s" % (c, _wconst(r)) if k < 0.9 else "~/%s/" % c)
    rest = r.choice(["/[0-9 \\n]/", "/[0-9 \\n\\x80-\\xff]/", "/[^a-zA-N]/"])
    return "(%s | %s)" % (" | ".join(alts), rest)


WIDE_ALPHABET = (WIDE + "0 \n").encode() + b"\xff\xc3\xa9"


def program_wide(seed):
    """The grammar shapes of program() over 40 letters and the bytes from 0x80 on, constants of 1, 2-16 and 17-40 bytes; about a third
    of the seeds are letter tables (more than 31 byte classes); about a third run a second stage that accepts every input, so that an
    input sampled from the first stage's transducer is one the whole pipeline accepts.  Sample with alphabet=WIDE_ALPHABET."""
    r = random.Random(seed * 104729 + 7)
    if r.random() < 0.35:
        body = _letter_table(r)
        if r.random() < 0.4:
            body = "%s %s" % (body, _wterm(r, 1))
    else:
        body = _wterm(r, 3)
    k = r.random()
    if k < 0.55:
        src = "main := (%s)*\n" % body
    elif k < 0.80:
        src = "main := (part /\\n/)*\npart := %s\n" % body
    else:
        src = "main := %s\n" % body
    if r.random() < 0.3:
        second = 'tidy := (~/%s/ %s | /./)*\n' % (r.choice("XYZ,"), _wconst(r))
        return "start: main >> tidy\n" + src + second
    return src


def first_stage(src):
    """the first stage of a program_wide() pipeline as a program of its own (any other program: itself)"""
    if not src.startswith("start:"):
        return src
    return "".join(src.splitlines(True)[1:-1])


# ---------------------------------------------------------------------------------------------------- register actions
REGS = "pqr"


def _aitem(r, regs):
    c = r.random()
    if c < 0.30:
        return "%s@(%s)" % (r.choice(regs), _term(r, 1))
    if c < 0.50:
        return "!%s" % r.choice(regs)
    if c < 0.56:
        return '[%s <- "%s"]' % (r.choice(regs), r.choice(["", "X", "YZ,"]))
    if c < 0.62:
        return '[%s += %s "%s"]' % (r.choice(regs), r.choice(regs), r.choice("XYZ,"))
    if c < 0.70:
        return "%s@(%s@(%s) %s)" % (regs[0], regs[1], _term(r, 1), _term(r, 0))
    return _term(r, 1)


def _aseq(r, regs):
    items = [_aitem(r, regs) for _ in range(r.randint(2, 5))]
    if r.random() < 0.3:
        k = r.randrange(len(items))
        items[k] = "(%s | %s)" % (items[k], _aitem(r, regs))
    return " ".join(items)


def program_actions(seed):
    """Bodies of r@(term), !r, [r <- …], [r += …] and plain terms over three registers, inside a star.  Shapes:
      lines   every register is written out in front of the line end: the post-pass finds a safe cut point behind every line;
      loose   whatever the body leaves in its registers stays there over the star: safe points where they happen to be empty;
      alive   a register filled in front of the star and written behind it: no safe point, the one-wave replay;
      framed  one redirect around the whole star: no safe point either."""
    r = random.Random(seed * 15485863 + 11)
    body = _aseq(r, REGS)
    k = r.random()
    if k < 0.40:
        return "main := (%s %s /\\n/)*\n" % (body, " ".join("!" + x for x in r.sample(REGS, 3)))
    if k < 0.65:
        return "main := (%s)*\n" % body if r.random() < 0.5 else "main := (%s /\\n/)*\n" % body
    if k < 0.85:
        return "main := k@(/[abc]/) (%s /\\n/)* !k\n" % body
    return 'main := k@((%s /\\n/)*) "<" !k ">"\n' % body
