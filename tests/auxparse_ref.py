"""An independent restatement of include/pcabi.h "SAM tags read from FASTQ / FASTA headers": what a header's
tab-separated TG:T:value fields parse to as BAM aux bytes. Plain Python: re, struct, and float(text) packed as
'<f'. Nothing here looks at the library."""
import math
import re
import struct

NAME = re.compile(rb'[A-Za-z][A-Za-z0-9]\Z')
INT = re.compile(rb'[-+]?[0-9]{1,10}\Z')
FLOAT = re.compile(rb'([-+]?[0-9]*\.?[0-9]+([eE][-+]?[0-9]+)?|[-+]?inf|[-+]?nan)\Z')
PRINTABLE = re.compile(rb'[\x20-\x7e]*\Z')
HEX = re.compile(rb'([0-9A-Fa-f]{2})*\Z')
RANGE = {'c': (-128, 127), 'C': (0, 255), 's': (-32768, 32767), 'S': (0, 65535), 'i': (-2 ** 31, 2 ** 31 - 1), 'I': (0, 2 ** 32 - 1)}
FMT = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I', 'f': '<f'}


def float_bytes(text):
    """float32 of C's (float)strtod(text): the double rounded to nearest, past the largest float an infinity."""
    x = float(text.decode())
    try:
        return struct.pack('<f', x)
    except OverflowError:
        return struct.pack('<f', math.copysign(math.inf, x))


def is_float(text):
    return len(text) <= 31 and FLOAT.match(text) is not None


def int_tag(text):
    """(type letter, value) of an i field's text, or None."""
    if not INT.match(text):
        return None
    v = int(text)
    if text[:1] == b'-':
        if v < -2 ** 31:
            return None
        return ('c' if v >= -128 else 's' if v >= -32768 else 'i'), v
    if v > 2 ** 32 - 1:
        return None
    return ('C' if v <= 255 else 'S' if v <= 65535 else 'I'), v


def field(f):
    """The aux bytes of one candidate field, or None when it is left out."""
    if len(f) < 5 or not NAME.match(f[:2]) or f[2:3] != b':' or f[4:5] != b':':
        return None
    tag, typ, v = f[:2], chr(f[3]), f[5:]
    if typ == 'A':
        return tag + b'A' + v if len(v) == 1 and PRINTABLE.match(v) else None
    if typ == 'i':
        t = int_tag(v)
        return None if t is None else tag + t[0].encode() + struct.pack(FMT[t[0]], t[1])
    if typ == 'f':
        return tag + b'f' + float_bytes(v) if is_float(v) else None
    if typ == 'Z':
        return tag + b'Z' + v + b'\0' if PRINTABLE.match(v) else None
    if typ == 'H':
        return tag + b'H' + v + b'\0' if HEX.match(v) else None
    if typ == 'B':
        if len(v) < 1 or chr(v[0]) not in FMT:
            return None
        sub = chr(v[0])
        if len(v) == 1:
            elems = []
        elif v[1:2] != b',':
            return None
        else:
            elems = v[2:].split(b',')
        out = []
        for e in elems:
            if sub == 'f':
                if not is_float(e):
                    return None
                out.append(float_bytes(e))
            else:
                if not INT.match(e) or not RANGE[sub][0] <= int(e) <= RANGE[sub][1]:
                    return None
                out.append(struct.pack(FMT[sub], int(e)))
        return tag + b'B' + sub.encode() + struct.pack('<I', len(out)) + b''.join(out)
    return None


def parse(header):
    """(chain, tags read, fields left out) of a header (the text after '@' / '>', without the line end)."""
    chain, tags, left_out = b'', 0, 0
    for f in header.split(b'\t')[1:]:
        a = field(f)
        if a is None:
            left_out += 1
        else:
            chain += a
            tags += 1
    return chain, tags, left_out


def walk(chain):
    """[(tag, type, subtype or '', value bytes)] of a chain this module made."""
    out, at = [], 0
    while at < len(chain):
        tag, typ = chain[at:at + 2], chr(chain[at + 2])
        at += 3
        if typ in 'ZH':
            z = chain.index(b'\0', at)
            out.append((tag, typ, '', chain[at:z]))
            at = z + 1
        elif typ == 'B':
            sub, n = chr(chain[at]), struct.unpack_from('<I', chain, at + 1)[0]
            w = struct.calcsize(FMT[sub])
            out.append((tag, typ, sub, chain[at + 5:at + 5 + n * w]))
            at += 5 + n * w
        else:
            w = 1 if typ == 'A' else struct.calcsize(FMT[typ])
            out.append((tag, typ, '', chain[at:at + w]))
            at += w
    return out


def same_chain(got, want):
    """Byte equality, except that a NaN compares as a NaN: float values that are both NaN are equal."""
    if got == want:
        return True
    if len(got) != len(want):
        return False
    try:
        a, b = walk(got), walk(want)
    except (ValueError, IndexError, KeyError, struct.error):
        return False
    if len(a) != len(b):
        return False
    for (t0, y0, s0, v0), (t1, y1, s1, v1) in zip(a, b):
        if (t0, y0, s0, len(v0)) != (t1, y1, s1, len(v1)):
            return False
        if y0 == 'f' or s0 == 'f':
            for k in range(0, len(v0), 4):
                x, y = struct.unpack_from('<f', v0, k)[0], struct.unpack_from('<f', v1, k)[0]
                if not (v0[k:k + 4] == v1[k:k + 4] or (math.isnan(x) and math.isnan(y))):
                    return False
        elif v0 != v1:
            return False
    return True
