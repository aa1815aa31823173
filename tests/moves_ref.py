"""A plain-Python restatement of the move-table rule (mv / ts remapped onto parts of a read) for the remap
tests (test_moves_cpu.py, test_gpu_moves.py). TEST INFRASTRUCTURE ONLY: nothing here is computed by the
code under test, and nothing of the library is imported.

mv is a B:c (or B:C) array: the stride S, then n moves of 0 or 1; a 1 starts a base. p(k) is the index
of the k-th 1 (from 0), p(ones) = n. A part [s0, s0 + ns) takes the moves [q0, q1): q0 = 0 when s0 == 0,
else p(s0); q1 = p(s0 + ns). It is written as `mv B c`, the count, S and the slice, then `ts i` with
ts + S * q0 when the read had a ts."""
import struct

INT32_MAX = 2 ** 31 - 1
WIDTH = {'c': 1, 'C': 1, 's': 2, 'S': 2, 'i': 4, 'I': 4, 'f': 4}
INT_FMT = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I'}
MODS = (b'MM', b'ML', b'MN', b'Mm', b'Ml')


def walk_aux(aux):
    """[(tag, type, raw bytes of the whole field)] of an aux chain."""
    out, at = [], 0
    while at < len(aux):
        tag, typ = aux[at:at + 2], chr(aux[at + 2])
        if typ in 'AcC':
            end = at + 4
        elif typ in 'sS':
            end = at + 5
        elif typ in 'iIf':
            end = at + 7
        elif typ in 'ZH':
            end = aux.index(b'\0', at + 3) + 1
        else:
            assert typ == 'B'
            end = at + 8 + WIDTH[chr(aux[at + 3])] * struct.unpack_from('<I', aux, at + 4)[0]
        out.append((tag, typ, aux[at:end]))
        at = end
    return out


def moves_of_aux(aux):
    """(vals, ts, bad) of an aux chain, or None when it has no mv tag. vals: the array's values as a list
    (stride first; [] when the chain shows the tag unusable); ts: the value, None without the tag; bad:
    what the chain alone shows -- mv twice or not B:c / B:C, ts twice, not an integer, negative or above
    INT32_MAX."""
    vals, ts, bad, n_mv, n_ts = [], None, False, 0, 0
    for tag, typ, raw in walk_aux(aux):
        if tag == b'mv':
            n_mv += 1
            if typ != 'B' or raw[3:4] not in (b'c', b'C'):
                bad = True
            else:
                vals = list(raw[8:])          # as bytes: a negative c value is >= 128
        elif tag == b'ts':
            n_ts += 1
            if typ not in INT_FMT:
                bad = True
            else:
                ts = struct.unpack_from(INT_FMT[typ], raw, 3)[0]
                if ts < 0 or ts > INT32_MAX:
                    bad = True
    if n_mv == 0:
        return None
    if n_mv > 1 or n_ts > 1:
        bad = True
    return ([] if bad else vals), ts, bad


def p_of(moves, k):
    """The index of the k-th 1 (from 0); len(moves) for k = the number of ones."""
    ones = [i for i, m in enumerate(moves) if m == 1]
    assert 0 <= k <= len(ones)
    return ones[k] if k < len(ones) else len(moves)


def slice_of(moves, s0, ns):
    q0 = 0 if s0 == 0 else p_of(moves, s0)
    return q0, p_of(moves, s0 + ns)


def usable(vals, ts, bad, l_seq, parts):
    """The rule's usability list, for a read of l_seq bases written as `parts` [(s0, ns)]."""
    if bad or len(vals) < 1 or not 1 <= vals[0] <= 127:
        return False
    moves = vals[1:]
    if len(moves) > INT32_MAX or any(m not in (0, 1) for m in moves) or sum(moves) != l_seq:
        return False
    if ts is not None:
        for s0, ns in parts:
            if ts + vals[0] * slice_of(moves, s0, ns)[0] > INT32_MAX:
                return False
    return True


def part_tags(vals, ts, s0, ns):
    """A usable read's part: its mv bytes, then its ts bytes."""
    moves = vals[1:]
    q0, q1 = slice_of(moves, s0, ns)
    out = b'mvBc' + struct.pack('<I', 1 + q1 - q0) + bytes([vals[0]]) + bytes(moves[q0:q1])
    if ts is not None:
        out += b'tsi' + struct.pack('<i', ts + vals[0] * q0)
    return out


def read_tags(aux, l_seq, parts):
    """[tag bytes of every part] by the table-level rule: b'' for all of them when the read is not usable;
    and whether it is."""
    got = moves_of_aux(aux)
    if got is None or not usable(*got, l_seq, parts):
        return [b''] * len(parts), False
    return [part_tags(got[0], got[1], s0, ns) for s0, ns in parts], True


def part_aux(aux, l_seq, parts, k, verbatim, keep_moves=True, mods=b''):
    """The aux chain of written part k of `parts`: verbatim: the part is its whole read with bases as
    stored; mods: the part's remapped MM ML MN bytes (keep_mods), which stand before mv."""
    if verbatim:
        return aux
    got = moves_of_aux(aux)
    ok = keep_moves and got is not None and usable(*got, l_seq, parts)
    new_ts = ok and got[1] is not None
    kept = b''.join(raw for tag, _, raw in walk_aux(aux) if tag not in MODS and tag != b'mv' and not (new_ts and tag == b'ts'))
    return kept + mods + (part_tags(got[0], got[1], *parts[k]) if ok else b'')
