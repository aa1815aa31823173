"""CPU restatement of approx_counter's two counting steps (TEST INFRASTRUCTURE ONLY), used to
check custom_porechop_abi_amd/approx_counter.py's host logic without a GPU. Pinned by
tests/golden/g5_kmer.json.gz (the reference program's own outputs).
  count_kmers : porechop_abi/ab_initio_src/approx_counter.cpp:487-519 (with is_DNA :313-321,
                haveLowComplexity :214-234, isForbiddenKmer :330-332)
  error_count : :531-601 as sum over sequences of 3 - d for the best substring edit distance
                d <= 2 (best_distances: a plain DP, free text start, minimum over text ends).
Both are vectorised over positions / k-mers so that the kernel tests (tests/kmer_cases.py) can afford
them; best_distances_plain keeps the cell-by-cell recurrence, and tests/test_kmer_core_cpu.py checks the
two against each other. tests/golden/g5_kmer_edge.json.gz pins the restatement at k 4 .. 32."""
import numpy as np


def _seqs(samples):
    return [samples.codes[o:o + n] for o, n in zip(samples.offs.tolist(), samples.lens.tolist())]


def window_values(samples, k):
    """Every window of every sequence, in sequence then position order: (2-bit value, first base in the
    top bits; holds no N)."""
    vals, dna = [np.zeros(0, np.uint64)], [np.zeros(0, bool)]
    for s in _seqs(samples):
        n = len(s) - k + 1
        if n <= 0:
            continue
        s = s.astype(np.uint64)
        v, ok = np.zeros(n, np.uint64), np.ones(n, bool)
        for i in range(k):
            ok &= s[i:i + n] < 4
            v = (v << np.uint64(2)) | (s[i:i + n] & np.uint64(3))
        vals.append(v)
        dna.append(ok)
    return np.concatenate(vals), np.concatenate(dna)


def dimer_score(v, k):
    """haveLowComplexity's score in float32: sum over the 16 dimers of c (c - 1) for the k - 1 dimers of
    the k-mer, / float(2 (k - 2)). NaN (0 / 0) at k = 2."""
    v = np.asarray(v, np.uint64)
    dim = [(v >> np.uint64(2 * i)) & np.uint64(15) for i in range(k - 1)]
    tot = np.zeros(len(v), np.int64)
    for d in range(16):
        c = np.zeros(len(v), np.int64)
        for x in dim:
            c += x == np.uint64(d)
        tot += c * (c - 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return tot.astype(np.float32) / np.float32(2 * (k - 2))


def count_kmers(samples, k, threshold, forbidden=(), device=0):
    v, dna = window_values(samples, k)
    forb = np.array(sorted(set(int(x) for x in forbidden)), np.uint64)
    with np.errstate(invalid='ignore'):
        low = dimer_score(v, k) >= np.float32(threshold)   # NaN: not low-complexity, the reference's float compare
    keys, counts = np.unique(v[dna & ~low & ~np.isin(v, forb)], return_counts=True)
    return keys.astype(np.uint64), counts.astype(np.int64)


def _padded(samples):
    seqs = _seqs(samples)
    ln = np.array([len(s) for s in seqs], np.int64)
    a = np.full((len(seqs), max(ln.tolist() + [1])), 4, np.int8)
    for i, s in enumerate(seqs):
        a[i, :len(s)] = s
    return a, ln


def _patterns(kmers, k):
    km = np.asarray(kmers, np.uint64).reshape(-1)
    return np.stack([((km >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)).astype(np.int8) for i in range(k)], axis=1)


def best_distances_plain(samples, kmers, k):
    """best[q, s]: the least edit distance of k-mer q to a substring of sequence s (k for an empty one).
    D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (text j != pattern i), D[i-1][j] + 1,
    D[i][j-1] + 1), cell by cell; an N matches nothing."""
    a, ln = _padded(samples)
    out = np.zeros((len(np.asarray(kmers).reshape(-1)), len(ln)), np.int64)
    for q, pat in enumerate(_patterns(kmers, k).tolist()):
        prev = np.tile(np.arange(k + 1), (len(ln), 1))
        best = np.full(len(ln), k)
        for j in range(a.shape[1]):
            c = a[:, j]
            cur = np.zeros_like(prev)
            for i in range(1, k + 1):
                cur[:, i] = np.minimum(np.minimum(prev[:, i - 1] + (c != pat[i - 1]), prev[:, i] + 1), cur[:, i - 1] + 1)
            live = j < ln
            best = np.where(live, np.minimum(best, cur[:, k]), best)
            prev = np.where(live[:, None], cur, prev)
        out[q] = best
    return out


def best_distances(samples, kmers, k):
    """best_distances_plain over all k-mers at once. Within a column the step from the row above,
    cur[i] = min(t[i], cur[i - 1] + 1) with t[i] = min(prev[i - 1] + mismatch, prev[i] + 1), t[0] = 0,
    unrolls to cur[i] = i + min over r <= i of (t[r] - r): a running minimum."""
    a, ln = _padded(samples)
    pat = _patterns(kmers, k)
    idx = np.arange(k + 1, dtype=np.int16)
    out = np.zeros((len(pat), len(ln)), np.int64)
    step = max(1, 2000000 // (len(ln) * (k + 1) + 1))
    for q0 in range(0, len(pat), step):
        p = pat[q0:q0 + step]
        prev = np.broadcast_to(idx, (len(p), len(ln), k + 1)).copy()
        best = np.full((len(p), len(ln)), k, np.int16)
        for j in range(a.shape[1]):
            t = np.zeros_like(prev)
            t[..., 1:] = np.minimum(prev[..., :-1] + (p[:, None, :] != a[None, :, j, None]), prev[..., 1:] + 1)
            cur = np.minimum.accumulate(t - idx, axis=-1) + idx
            live = j < ln
            best = np.where(live[None, :], np.minimum(best, cur[..., k]), best)
            prev = np.where(live[None, :, None], cur, prev)
        out[q0:q0 + len(p)] = best
    return out


def error_count(samples, kmers, k, device=0):
    best = best_distances(samples, kmers, k)
    return np.where(best <= 2, 3 - best, 0).sum(axis=1).astype(np.int64)


def count_kmers_top(samples, k, threshold, forbidden=(), top=0, min_count=0, device=0):
    """pcabi_kmer_top_host restated: count_kmers, then count descending (ties k-mer ascending),
    only the entries with count >= max(min_count, the top-th largest count)."""
    import numpy as np
    km, cn = count_kmers(samples, k, threshold, forbidden, device)
    km = np.asarray(km, np.uint64)
    cn = np.asarray(cn, np.int64)
    order = np.lexsort((km, -cn))
    km, cn = km[order], cn[order]
    thr = max(int(min_count), 0)
    if 0 < top <= len(cn):
        thr = max(thr, int(cn[top - 1]))
    keep = cn >= thr
    return km[keep], cn[keep]
