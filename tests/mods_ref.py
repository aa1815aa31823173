"""A plain-Python restatement of the base-modification tag rules (SAMtags "Base modifications") for the
remap tests (test_mods_cpu.py, test_gpu_mods.py). TEST INFRASTRUCTURE ONLY: nothing here is computed by
the code under test, and nothing of the library is imported.

decode() turns MM / ML against a sequence into explicit records (position, base, strand, code,
probability); slice_records() cuts and shifts them for a part; encode_part() writes a part's tags by the
project's canonical rule (header verbatim, first kept count recomputed, later counts byte for byte,
empty groups kept); part_aux() is the whole aux chain a written part must carry."""
import re
import struct

GROUP = re.compile(rb'([ACGTUN])([+-])([a-z]+|[0-9]+)([.?]?)((?:,[0-9]+)*);')
INT32_MAX = 2 ** 31 - 1
MAX_GROUPS = 32
POSITIONAL = (b'MM', b'ML', b'MN', b'Mm', b'Ml', b'mv')


def parse_mm(mm):
    """[(header bytes, base, strand, codes, [count texts])] or None when the text is not well formed."""
    groups, pos = [], 0
    while pos < len(mm):
        m = GROUP.match(mm, pos)
        if m is None:
            return None
        base, strand, codes, flag, counts = m.groups()
        code_list = [codes.decode()] if codes.isdigit() else [chr(c) for c in codes]
        texts = counts.split(b',')[1:] if counts else []
        groups.append((base + strand + codes + flag, base.decode(), strand.decode(), code_list, texts))
        pos = m.end()
    return groups


def occurrences(seq, base):
    """Positions of the base a group counts: its own letter, T for U, every position for N."""
    if base == 'N':
        return list(range(len(seq)))
    want = 'T' if base == 'U' else base
    return [i for i, c in enumerate(seq) if c == want]


def resolve(seq, mm, ml, mn):
    """The groups of a usable read as [(header, base, strand, codes, texts, ordinals, positions, ml0)],
    or None when the tags are not usable. seq: str; mm: bytes; ml: bytes or None; mn: int or None."""
    if mm is None:
        return None
    groups = parse_mm(mm)
    if groups is None or len(groups) > MAX_GROUPS:
        return None
    out, ml_at = [], 0
    for header, base, strand, codes, texts in groups:
        occ = occurrences(seq, base)
        ords, o = [], -1
        for t in texts:
            d = int(t)
            if d > INT32_MAX:
                return None
            o = o + 1 + d
            ords.append(o)
        if ords and ords[-1] >= len(occ):
            return None
        out.append((header, base, strand, codes, texts, ords, [occ[o] for o in ords], ml_at))
        ml_at += len(ords) * len(codes)
    if ml is not None and len(ml) != ml_at:
        return None
    if mn is not None and mn != len(seq):
        return None
    return out


def decode(seq, mm, ml, mn):
    """Sorted [(position, base, strand, code, probability or None)], or None when not usable."""
    groups = resolve(seq, mm, ml, mn)
    if groups is None:
        return None
    recs = []
    for header, base, strand, codes, texts, ords, positions, ml0 in groups:
        for k, p in enumerate(positions):
            for c, code in enumerate(codes):
                recs.append((p, base, strand, code, None if ml is None else ml[ml0 + k * len(codes) + c]))
    return sorted(recs, key=lambda r: (r[0], r[1], r[2], r[3], -1 if r[4] is None else r[4]))


def slice_records(recs, s0, ns):
    return [(r[0] - s0,) + r[1:] for r in recs if s0 <= r[0] < s0 + ns]


def encode_part(seq, mm, ml, mn, s0, ns):
    """(MM text, ML values or None, MN or None) of part [s0, s0 + ns) of a usable read."""
    groups = resolve(seq, mm, ml, mn)
    assert groups is not None
    text, vals = b'', b''
    for header, base, strand, codes, texts, ords, positions, ml0 in groups:
        occ = occurrences(seq, base)
        c0 = sum(1 for p in occ if p < s0)
        c1 = sum(1 for p in occ if p < s0 + ns)
        keep = [k for k, o in enumerate(ords) if c0 <= o < c1]
        text += header
        for n, k in enumerate(keep):
            text += b',' + (str(ords[k] - c0).encode() if n == 0 else texts[k])
            if ml is not None:
                vals += ml[ml0 + k * len(codes):ml0 + (k + 1) * len(codes)]
        text += b';'
    return text, (vals if ml is not None else None), (ns if mn is not None else None)


# ---- aux chains -------------------------------------------------------------------------------------
WIDTH = {'A': 1, 'c': 1, 'C': 1, 's': 2, 'S': 2, 'i': 4, 'I': 4, 'f': 4}


def walk_aux(aux):
    """[(tag, type, whole tag bytes)]."""
    out, at = [], 0
    while at < len(aux):
        tag, typ = aux[at:at + 2], chr(aux[at + 2])
        if typ in WIDTH:
            end = at + 3 + WIDTH[typ]
        elif typ in 'ZH':
            end = aux.index(b'\0', at + 3) + 1
        else:
            assert typ == 'B'
            end = at + 8 + WIDTH[chr(aux[at + 3])] * struct.unpack_from('<I', aux, at + 4)[0]
        out.append((tag, typ, aux[at:end]))
        at = end
    return out


def mods_of_aux(aux):
    """(mm, ml, mn, mm_tag, ml_tag, bad) of an aux chain; the first three None when absent. bad: what the
    chain alone shows to be unusable (not exactly one MM among MM / Mm, a tag twice, a wrong type)."""
    mm = ml = mn = None
    mm_tag, ml_tag = b'MM', b'ML'
    n = {b'MM': 0, b'ML': 0, b'MN': 0}
    bad = False
    for tag, typ, raw in walk_aux(aux):
        key = tag.upper() if tag in (b'Mm', b'Ml') else tag
        if key not in n:
            continue
        n[key] += 1
        if key == b'MM':
            if typ != 'Z':
                bad = True
            else:
                mm, mm_tag = raw[3:-1], tag
        elif key == b'ML':
            if typ != 'B' or raw[3:4] != b'C':
                bad = True
            else:
                ml, ml_tag = raw[8:], tag
        else:
            fmt = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I'}.get(typ)
            if fmt is None:
                bad = True
            else:
                mn = struct.unpack_from(fmt, raw, 3)[0]
                if mn < 0 or mn > INT32_MAX:
                    bad = True
    if n[b'MM'] != 1 or n[b'ML'] > 1 or n[b'MN'] > 1:
        bad = True
    return mm, ml, mn, mm_tag, ml_tag, bad


def has_mods(aux):
    return any(tag in POSITIONAL[:5] for tag, _, _ in walk_aux(aux))


def read_usable(seq, aux):
    mm, ml, mn, _, _, bad = mods_of_aux(aux)
    return not bad and resolve(seq, mm, ml, mn) is not None


def tag_bytes(text, vals, mn, mm_tag=b'MM', ml_tag=b'ML'):
    out = mm_tag + b'Z' + text + b'\0'
    if vals is not None:
        out += ml_tag + b'BC' + struct.pack('<I', len(vals)) + vals
    if mn is not None:
        out += b'MNi' + struct.pack('<i', mn)
    return out


def part_aux(seq, aux, s0, ns, verbatim, keep_mods=True):
    """The aux chain of a written part: seq = the read in the reader's orientation, aux = its record's
    chain; verbatim: the part is its whole read with bases as stored."""
    if verbatim:
        return aux
    kept = b''.join(raw for tag, _, raw in walk_aux(aux) if tag not in POSITIONAL)
    if not keep_mods or not has_mods(aux) or not read_usable(seq, aux):
        return kept
    mm, ml, mn, mm_tag, ml_tag, _ = mods_of_aux(aux)
    return kept + tag_bytes(*encode_part(seq, mm, ml, mn, s0, ns), mm_tag, ml_tag)


def decode_aux(seq, aux):
    """decode() of the modification tags in an aux chain ([] when it has none); None when not usable."""
    if not has_mods(aux):
        return []
    mm, ml, mn, _, _, bad = mods_of_aux(aux)
    return None if bad else decode(seq, mm, ml, mn)
