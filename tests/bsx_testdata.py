"""Seeded synthetic genomes and bisulfite reads for the parity tests (small sizes, pure numpy)."""
import numpy as np

COMP = bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn")


def revcomp(s: str) -> str:
    return s.encode().translate(COMP)[::-1].decode()


def random_seq(rng, n, gc=0.5):
    p = [(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, size=n, p=p)]


def make_genome(seed=1, chr_lens=(1_000_000,), gc=0.51, n_runs=6, repeats=20, microsats=10, lower=4, iupac=5, cpg_sites=0,
                digest="CCGG"):
    """returns list of (name, str).  Features that the reference treats specially are all present:
    N runs (block breaks), short islands (<30 nt, dropped), lower-case stretches, IUPAC codes (packed as A),
    dispersed repeats, (TG)n / poly-T microsatellites (huge 3-letter buckets)."""
    rng = np.random.default_rng(seed)
    out = []
    fam = random_seq(rng, 300, gc)
    for ci, L in enumerate(chr_lens):
        s = random_seq(rng, L, gc).copy()
        for _ in range(repeats):  # dispersed repeat family, ~8 % divergence
            ln = int(rng.integers(120, 300))
            pos = int(rng.integers(0, max(1, L - ln)))
            cp = fam[:ln].copy()
            mut = rng.random(ln) < 0.08
            cp[mut] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(mut.sum()))]
            if rng.random() < 0.5:
                cp = np.frombuffer(cp.tobytes().translate(COMP)[::-1], dtype=np.uint8)
            s[pos:pos + ln] = cp
        for k in range(microsats):
            ln = int(rng.integers(40, 400))
            pos = int(rng.integers(0, max(1, L - ln)))
            unit = [b"TG", b"T", b"CA", b"A", b"TTG"][k % 5]
            s[pos:pos + ln] = np.frombuffer((unit * (ln // len(unit) + 1))[:ln], dtype=np.uint8)
        for _ in range(cpg_sites):  # RRBS: sprinkle digestion sites
            pos = int(rng.integers(0, max(1, L - 8)))
            s[pos:pos + len(digest)] = np.frombuffer(digest.encode(), dtype=np.uint8)
        for _ in range(lower):
            ln = int(rng.integers(50, 2000))
            pos = int(rng.integers(0, max(1, L - ln)))
            s[pos:pos + ln] |= 0x20
        for _ in range(iupac):
            pos = int(rng.integers(0, L))
            s[pos] = b"RYMKSW"[int(rng.integers(0, 6))]
        for k in range(n_runs):
            ln = int(rng.integers(1, 3000)) if k % 2 else int(rng.integers(1, 6))
            pos = int(rng.integers(0, max(1, L - ln)))
            s[pos:pos + ln] = ord("N") if k % 3 else ord("n")
            if k % 2 == 0 and pos + ln + 20 + 4 < L:  # a short island between two N runs (< 30 nt -> not indexed)
                s[pos + ln + 20:pos + ln + 24] = ord("N")
        if ci == 0 and L > 200:
            s[:37] = ord("N")  # leading Ns
        out.append((f"chr{ci + 1}", s.tobytes().decode()))
    return out


def write_fasta(path, genome, width=70, extra_header=" some description"):
    with open(path, "w") as f:
        for name, s in genome:
            f.write(f">{name}{extra_header}\n")
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + "\n")


def fasta_text(genome, width=70):
    parts = []
    for name, s in genome:
        parts.append(f">{name} desc\n")
        parts.extend(s[i:i + width] + "\n" for i in range(0, len(s), width))
    return "".join(parts)


def bs_convert(frag: str, rng, conv_nonCpG=0.995, conv_CpG=0.25):
    b = bytearray(frag.upper().encode())
    n = len(b)
    r = rng.random(n)
    for i in range(n):
        if b[i] == 67:  # C
            cpg = i + 1 < n and b[i + 1] == 71
            if r[i] < (conv_CpG if cpg else conv_nonCpG):
                b[i] = 84
    return b.decode()


def mutate(seq: str, rng, sub_rate=0.005, n_rate=0.0, max_subs=None):
    b = bytearray(seq.encode())
    n = len(b)
    r = rng.random(n)
    subs = np.nonzero(r < sub_rate)[0]
    if max_subs is not None:
        subs = subs[:max_subs]
    for i in subs:
        b[i] = b"ACGT"[(b"ACGT".find(bytes([b[i]])) + int(rng.integers(1, 4))) % 4] if bytes([b[i]]) in b"ACGT" else b[i]
    if n_rate > 0:
        for i in np.nonzero(rng.random(n) < n_rate)[0]:
            b[i] = ord("N")
    return b.decode()


def _sample_fragment(genome, rng, length):
    while True:
        ci = int(rng.integers(0, len(genome)))
        name, s = genome[ci]
        if len(s) < length + 2:
            continue
        pos = int(rng.integers(0, len(s) - length))
        frag = s[pos:pos + length]
        if frag.upper().count("N") > length // 2:
            continue
        return ci, pos, frag


def make_se_reads(genome, n, length, seed=1, sub_rate=0.005, n_rate=0.001, strands=("++", "-+"), var_len=False,
                  junk_frac=0.02, qual_tail=False, adapter=None):
    """returns list of dict(name, seq, qual, chr, pos, strand)"""
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n):
        L = int(rng.integers(max(20, length // 2), length + 1)) if var_len else length
        if rng.random() < junk_frac:
            seq = random_seq(rng, L).tobytes().decode()
            reads.append(dict(name=f"r{i}_junk", seq=seq, qual="I" * L, chr=-1, pos=-1, strand="*"))
            continue
        ci, pos, frag = _sample_fragment(genome, rng, L)
        strand = strands[int(rng.integers(0, len(strands)))]
        if strand[0] == "+":
            conv = bs_convert(frag, rng)
        else:
            conv = bs_convert(revcomp(frag.upper()), rng)
        seq = conv if strand[1] == "+" else revcomp(conv)
        seq = mutate(seq, rng, sub_rate, n_rate)
        qual = "I" * L
        if adapter is not None and rng.random() < 0.3:
            ins = int(rng.integers(min(30, L - 1), L))  # (the same draw for L > 30)
            seq = (seq[:ins] + adapter + random_seq(rng, L).tobytes().decode())[:L]
        if qual_tail:
            t = int(rng.integers(0, 60))
            if t:
                q = bytearray(qual.encode())
                q[L - t:] = bytes(int(x) for x in rng.integers(35, 49, t))
                qual = q.decode()
        reads.append(dict(name=f"r{i}_{genome[ci][0]}_{pos + 1}_{strand}", seq=seq, qual=qual, chr=ci, pos=pos, strand=strand))
    return reads


def make_pe_reads(genome, n, length, seed=1, ins_mean=300, ins_sd=50, ins_min=50, ins_max=480, sub_rate=0.005,
                  n_rate=0.001, junk_frac=0.02, qual_tail=False, adapter=None, var_len=False):
    """mate 1 from ++ / -+, mate 2 the reverse complement of the far end (+- / --)"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        ins = int(np.clip(rng.normal(ins_mean, ins_sd), ins_min, ins_max))
        ci, pos, frag = _sample_fragment(genome, rng, ins)
        watson = rng.random() < 0.5
        conv = bs_convert(frag if watson else revcomp(frag.upper()), rng)
        L1 = int(rng.integers(max(20, length // 2), length + 1)) if var_len else length
        L2 = int(rng.integers(max(20, length // 2), length + 1)) if var_len else length
        filler = random_seq(rng, 2 * length).tobytes().decode()
        ad = adapter if adapter is not None else ""
        m1 = (conv + ad + filler)[:L1]
        m2 = (revcomp(conv) + ad + filler)[:L2]
        if rng.random() < junk_frac:
            m2 = random_seq(rng, L2).tobytes().decode()
        m1 = mutate(m1, rng, sub_rate, n_rate)
        m2 = mutate(m2, rng, sub_rate, n_rate)
        q1, q2 = "I" * L1, "I" * L2
        if qual_tail:
            for which in (0, 1):
                L = (L1, L2)[which]
                t = int(rng.integers(0, 60))
                if t:
                    q = bytearray(b"I" * L)
                    q[L - t:] = bytes(int(x) for x in rng.integers(35, 49, t))
                    if which == 0:
                        q1 = q.decode()
                    else:
                        q2 = q.decode()
        pairs.append(dict(name=f"p{i}_{genome[ci][0]}_{pos + 1}_{'W' if watson else 'C'}_{ins}", seq1=m1, qual1=q1, seq2=m2,
                          qual2=q2, chr=ci, pos=pos, ins=ins, watson=watson))
    return pairs


def make_rrbs_reads(genome, n, length, seed=1, digest="CCGG", digest_pos=1, sub_rate=0.005, max_frag=220, min_frag=40):
    """reads starting at digestion sites (C-CGG): fragment = [site_i + pos, site_j + pos + ...)"""
    rng = np.random.default_rng(seed)
    reads = []
    sites = []
    for ci, (name, s) in enumerate(genome):
        u = s.upper()
        p = u.find(digest)
        lst = []
        while p >= 0:
            lst.append(p + digest_pos)
            p = u.find(digest, p + 1)
        sites.append(lst)
    tries = 0
    while len(reads) < n and tries < 50 * n:
        tries += 1
        ci = int(rng.integers(0, len(genome)))
        lst = sites[ci]
        if len(lst) < 2:
            continue
        k = int(rng.integers(0, len(lst) - 1))
        a, b = lst[k], lst[k + 1] + len(digest) - 2 * digest_pos
        if not (min_frag <= b - a <= max_frag):
            continue
        frag = genome[ci][1][a:b]
        watson = rng.random() < 0.5
        conv = bs_convert(frag if watson else revcomp(frag.upper()), rng)
        seq = mutate(conv[:length], rng, sub_rate, 0.0)
        if len(seq) < 20:
            continue
        reads.append(dict(name=f"rr{len(reads)}_{genome[ci][0]}_{a + 1}_{'W' if watson else 'C'}", seq=seq, qual="I" * len(seq),
                          chr=ci, pos=a, strand="++" if watson else "-+"))
    return reads


def write_fastq(path, reads, seq_key="seq", qual_key="qual"):
    with open(path, "w") as f:
        for r in reads:
            f.write(f"@{r['name']}\n{r[seq_key]}\n+\n{r[qual_key]}\n")


def c1_full_inputs(tmp):
    """BASELINE.json's configs[0] at its stated size: 1 Mb genome FASTA + 10 000 single-end 36 bp reads (200 of them of
    varying length, so that the planner-state leak of DESIGN.md §4 occurs); returns (fasta path, fastq path, sha256 of both
    texts).  tests/golden/c1_full.json.gz holds the real binary's SAM for exactly these files."""
    import hashlib
    import os
    g = make_genome(seed=1, chr_lens=(1_000_000,), gc=0.51)
    fa = os.path.join(tmp, "c1_genome.fa")
    write_fasta(fa, g)
    reads = make_se_reads(g, 9_800, 36, seed=101, sub_rate=0.01, strands=("++", "-+"))
    reads += make_se_reads(g, 200, 36, seed=102, sub_rate=0.04, strands=("++", "-+"), var_len=True)
    fq = os.path.join(tmp, "c1_reads.fq")
    write_fastq(fq, reads)
    h = hashlib.sha256(open(fa, "rb").read() + open(fq, "rb").read()).hexdigest()
    return fa, fq, h


# ---- directed boundary reads (tests/test_oracle_boundaries.py, tests/test_gpu_boundaries.py) --------------------------------------------
# Nothing below draws a read: every read is built from a position, fully converted, with placed mismatches, and carries a label
# (its class and its origin locus), so a test knows why the read is there and where it must (or must not) be found.

BOUNDARY_LENGTHS = (31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 95, 96, 97, 112, 127, 128, 129, 143, 144)
STRANDS4 = ("++", "-+", "+-", "--")
END_DISTANCES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48)


def _plain(rng, n):
    return random_seq(rng, n, 0.5).tobytes().decode()


def make_boundary_genome(seed=41):
    """random sequence without repeats, ten chromosomes: chrA begins with NNNNN; chrN carries N runs of 1 and 40 letters, islands of 29
    and 30 letters between runs and a run that reaches its last letter; lengths 29 (no block at all), 30, 47, 64, 4 992 (a multiple of
    16), 4 993; chrL is long enough for the FASTA text to pass 64 KB; chrZ closes the reference.
    returns (genome, n_runs) with n_runs = the [begin, end) of every N run of chrN"""
    rng = np.random.default_rng(seed)
    parts = [_plain(rng, 300), "N", _plain(rng, 200), "N" * 40, _plain(rng, 29), "NNN", _plain(rng, 30), "NNN", _plain(rng, 300), "N" * 25]
    runs, at = [], 0
    for p in parts:
        if p[0] == "N":
            runs.append((at, at + len(p)))
        at += len(p)
    g = [("chrA", "NNNNN" + _plain(rng, 1495)), ("chrN", "".join(parts)), ("chr29", _plain(rng, 29)), ("chr30", _plain(rng, 30)),
         ("chr47", _plain(rng, 47)), ("chr64", _plain(rng, 64)), ("chr4992", _plain(rng, 4992)), ("chr4993", _plain(rng, 4993)),
         ("chrL", _plain(rng, 70_001)), ("chrZ", _plain(rng, 6000))]
    return g, runs


def packed_letters(s):
    """the letters the packed reference holds for a chromosome text: anything but ACGT packs as A"""
    return "".join(c if c in "ACGT" else "A" for c in s.upper())


def directed_read(text, strand, subs=(), n_at=()):
    """the read of `strand` over the forward-strand letters `text`: complete C->T conversion of the chosen strand ('+x' the text, '-x' its
    reverse complement), read as is ('x+') or reverse-complemented ('x-': a G->A read, which needs -n 1).  subs / n_at are READ positions:
    each sub becomes a change the 3-letter comparison must count (G<->A in a C->T read, C<->T in a G->A read) at the nearest position
    that can carry one and is still free; n_at positions become N"""
    conv = bytearray((text if strand[0] == "+" else revcomp(text)).replace("C", "T").encode())
    L = len(conv)
    flip = strand[1] == "-"
    used = set()
    for p in subs:
        q = L - 1 - p if flip else p
        for d in range(L):
            c = [x for x in (q + d, q - d) if 0 <= x < L and x not in used and conv[x] in b"GA"]
            if c:
                used.add(c[0])
                conv[c[0]] = ord("A") if conv[c[0]] == ord("G") else ord("G")
                break
    for p in n_at:
        conv[L - 1 - p if flip else p] = ord("N")
    seq = conv.decode()
    return revcomp(seq) if flip else seq


def _rd(out, cls, genome, ci, pos, text, strand, **kw):
    seq = directed_read(text, strand, **kw)
    out.append(dict(name=f"{cls}_{len(out)}_{genome[ci][0]}_{pos}_{strand}_{len(seq)}", seq=seq, qual="I" * len(seq), cls=cls, chr=ci, pos=pos, strand=strand))


def _sub_layouts(n, L, s):
    """n placed mismatches in a read of L letters: at the head, at the tail, spread evenly, inside the second seed window"""
    if n == 0:
        return {"none": ()}
    return {"head": tuple(range(n)), "tail": tuple(range(L - n, L)), "even": tuple((2 * k + 1) * L // (2 * n) for k in range(n)),
            "seed": tuple(s + k % s for k in range(n))}


def boundary_se_reads(genome, runs, s=16, v=4, f=5, strands=STRANDS4):
    """classes A (ends), B (overhang), C (N runs and blocks), D (lengths), E (mismatches), F (N in the read) of single-end reads.  Labels:
    'A', 'B0' (flush, the overhang class's own control), 'Brand' / 'Bpack' (sticking out; the outside letters random / what the packed array
    holds there), 'C', 'D', 'E<n>' (n mismatches; 'Eover' = v + 1), 'F<n>' (n N letters; 'Fover' = f + 1)"""
    out = []
    rng = np.random.default_rng(97)
    P = [packed_letters(t) for _, t in genome]
    for ci, p in enumerate(P):                                               # A: every chromosome, both ends
        for L in (20, 100):
            for d in END_DISTANCES:
                for pos in (d, len(p) - L - d):
                    if 0 <= pos and pos + L <= len(p):
                        for st in strands:
                            _rd(out, "A", genome, ci, pos, p[pos:pos + L], st)
    L = 50                                                                   # B: sticking out in front of or behind the chromosome
    for ci, p in enumerate(P):
        if len(p) < 64:
            continue
        prev = ("A" * 48 + P[ci - 1] if ci else "") + "A" * 48               # what lies in front of letter 0: the neighbour, then at least 32 pad letters
        nxt = "A" * (32 + (-len(p)) % 16) + (P[ci + 1] if ci + 1 < len(P) else "") + "A" * 64
        for k in (0, 1, 2, 5, 16, 17, 33, 48):
            for variant in ("rand", "pack"):
                if k in (0, 33, 48) and variant == "rand":
                    continue
                cls = "B0" if k == 0 else "B" + variant
                front = (_plain(rng, k) if variant == "rand" else prev[len(prev) - k:]) + p[:L - k]
                behind = p[len(p) - (L - k):] + (_plain(rng, k) if variant == "rand" else nxt[:k])
                for st in strands:
                    _rd(out, cls, genome, ci, -k, front, st)
                    _rd(out, cls, genome, ci, len(p) - (L - k), behind, st)
    ci, p = 1, P[1]                                                          # C: chrN's runs and islands
    for L in (36, 100):
        for a, b in runs:
            for pos in [a + d - L for d in (-2, -1, 0, 1, 2)] + [b + d for d in (-1, 0, 1)]:
                if 0 <= pos and pos + L <= len(p):
                    for st in strands:
                        _rd(out, "C", genome, ci, pos, p[pos:pos + L], st)
    for (_, e0), (b1, _) in zip(runs[1:3], runs[2:4]):                       # the 29- and 30-letter islands
        for L in (20, b1 - e0):
            for pos in range(e0, b1 - L + 1):
                for st in strands:
                    _rd(out, "C", genome, ci, pos, p[pos:pos + L], st)
    spots = [(8, 0), (8, None), (6, 0), (6, None), (7, None), (8, 1000), (8, 1003), (9, 2017)]   # D: lengths (None = flush with the end)
    for L in sorted(set((s, s + 1) + BOUNDARY_LENGTHS + (145, 200))):
        for ci, pos in spots:
            pos = len(P[ci]) - L if pos is None else pos
            for st in strands:
                _rd(out, "D", genome, ci, pos, P[ci][pos:pos + L], st)
    mid = [(8, 5000), (8, 5021), (8, 12345), (9, 1000), (7, 2502), (0, 700)]
    L = 100
    for n in sorted({0, 1, v, v + 1}):                                       # E: placed mismatches
        for name, subs in _sub_layouts(n, L, s).items():
            for ci, pos in mid:
                for st in strands:
                    _rd(out, "Eover" if n == v + 1 else "E%d" % n, genome, ci, pos, P[ci][pos:pos + L], st, subs=subs)
    for n in (f - 1, f, f + 1):                                              # F: N letters in the read
        if n >= 0:
            for ci, pos in mid:
                for st in strands:
                    _rd(out, "Fover" if n == f + 1 else "F%d" % n, genome, ci, pos + 7, P[ci][pos + 7:pos + 7 + L], st, n_at=tuple((2 * k + 1) * L // (2 * n) for k in range(n)))
    return out


def boundary_pe_reads(genome, L=50, m=28, x=500):
    """class G: pairs of both fragment strands with placed inserts — m-2..m+1, L-1..L+1, 2L-1..2L+1, x-1..x+2 and whole chromosomes —
    and the fragment at letters 0, 1, 16, at the same distances from the end, and in the middle.  Mates are min(L, insert) long.  Labels
    'G' (insert inside [m, x]), 'Gunder', 'Gover'"""
    out = []
    P = [packed_letters(t) for _, t in genome]
    inserts = sorted({i for i in list(range(m - 2, m + 2)) + [L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1] + list(range(x - 1, x + 3)) if i >= 20})
    todo = []
    for ci in (0, 1, 6, 7, 8, 9):
        n = len(P[ci])
        for ins in inserts:
            for pos in (0, 1, 16, n // 2 + 3, n - ins - 16, n - ins - 1, n - ins):
                if 0 <= pos and pos + ins <= n:
                    todo.append((ci, pos, ins))
    todo += [(ci, 0, len(P[ci])) for ci in (3, 4, 5, 6, 0)]                    # the whole chromosome as the fragment
    for ci, pos, ins in todo:
        frag = P[ci][pos:pos + ins]
        Lr = min(L, ins)
        cls = "Gunder" if ins < m else "Gover" if ins > x else "G"
        for watson in (True, False):
            conv = (frag if watson else revcomp(frag)).replace("C", "T")
            m1, m2 = conv[:Lr], revcomp(conv)[:Lr]
            out.append(dict(name=f"{cls}_{len(out)}_{genome[ci][0]}_{pos}_{'W' if watson else 'C'}_{ins}", seq1=m1, qual1="I" * Lr, seq2=m2, qual2="I" * Lr,
                            cls=cls, chr=ci, pos=pos, ins=ins, watson=watson, locs=(pos, pos + ins - Lr)))
    return out


def make_boundary_rrbs_genome(m=40, x=220, digest="CCGG", digest_pos=1, seed=43):
    """digestion sites at letter 0 and in the last four letters, adjacent (CCGGCCGG), and at fragment sizes m-1, m, m+1, x-1, x, x+1 and
    4, 5, 8, 19..21 (fragment size = what the reference's CCGG_seglen gives a read inside one fragment: site distance + len(digest) -
    2 * digest_pos); a second chromosome of fragments spread over [m, x].  Random sequence without any other occurrence of the site; the
    longer fragments share their first and last 12 letters three ways, so that a site's index bucket holds many sites (the lists the heavy
    pipeline takes) while a read's origin stays its only good placement.
    returns (genome, sites): sites[c] = the cut positions (start of the occurrence + digest_pos), ascending"""
    rng = np.random.default_rng(seed)
    dl = len(digest)
    adj = dl - 2 * digest_pos

    heads = [_plain(rng, 12) for _ in range(3)]                               # fragments of 36 letters and more begin and end with one of three
    tails = [_plain(rng, 12) for _ in range(3)]                               # 12-mers: index buckets of many sites, one good placement per read

    def filler(n):
        while True:
            t = _plain(rng, n)
            if n >= 36:
                t = heads[n % 3] + t[12:-12] + tails[n // 3 % 3]
            if digest not in t and t[0] != digest[-1] and t[-1] != digest[0]:   # (no occurrence inside, none made where it meets a site)
                return t
            if n >= 36 and (heads[n % 3][0] == digest[-1] or tails[n // 3 % 3][-1] == digest[0] or digest in heads[n % 3] or digest in tails[n // 3 % 3]):
                heads[n % 3], tails[n // 3 % 3] = _plain(rng, 12), _plain(rng, 12)

    def chrom(sizes, tail=True):
        s = []
        for z in sizes:                                                      # z = fragment size -> distance of the occurrences z - adj
            d = z - adj
            assert d >= dl
            s.append(digest + (filler(d - dl) if d > dl else ""))
        s.append(digest if tail else digest + filler(37))
        return "".join(s)
    small = [d + adj for d in (4, 5, 8, 19, 20, 21)]                         # (distance 4: adjacent occurrences)
    sizes1 = [m - 1, 60, m, 75, m + 1, 90, x - 1, 50, x, 120, x + 1, 64] + small + [100, 77, 2 * x, 81, m - 1, x + 1, m - 1, x + 1, 66]
    sizes2 = [m + (x - m) * k // 23 for k in range(24)] + [x + 1 + k for k in range(8)] + [max(dl + adj, m - 1 - k) for k in range(8)]
    c1, c2 = chrom(sizes1), chrom(sizes2, tail=False)
    g = [("chrR1", c1), ("chrR2", c2)]
    sites = []
    for _, t in g:
        lst, p = [], t.find(digest)
        while p >= 0:
            lst.append(p + digest_pos)
            p = t.find(digest, p + 1)
        sites.append(lst)
    assert [len(x) for x in sites] == [len(sizes1) + 1, len(sizes2) + 1]
    return g, sites


def boundary_rrbs_reads(genome, sites, m=40, x=220, v=2, digest="CCGG", digest_pos=1, strands=STRANDS4):
    """class H: a read from every site in both directions, 20..144 letters, reads longer than their fragment and reads that run over the
    chromosome end (continued with the pad letters of the packed array) included.  Labels by the fragment size CCGG_seglen gives the read
    at its origin: 'H' inside [m, x], 'Hout' outside, 'Hend' where the read leaves the chromosome.  Reads of 75, 100 and 144 letters come
    a second and third time with v and v + 1 mismatches placed at their tail, behind letter 64 ('Hover' = v + 1)"""
    out = []
    dl = len(digest)
    adj = dl - 2 * digest_pos
    for ci, (_, t) in enumerate(genome):
        n = len(t)
        ext = "A" * 160 + t + "A" * 160
        ends = [sv + adj for sv in sites[ci]]
        for k, sv in enumerate(sites[ci]):
            for L in (20, 36, 50, 75, 100, 144):
                for fwd in (True, False):
                    pos = sv if fwd else ends[k] - L
                    text = ext[160 + pos:160 + pos + L]
                    if pos < 0 or pos + L > n:
                        cls = "Hend"
                    else:
                        left = [q for q in sites[ci] if q <= pos]
                        right = [e for e in ends if e >= pos + L]
                        if not right:
                            continue                                          # past the last site: the reference reads beyond its site vector
                        z = right[0] - (left[-1] if left else sites[ci][0])
                        cls = "H" if m <= z <= x else "Hout"
                    for st in strands:
                        if (st[0] == "+") == fwd:
                            _rd(out, cls, genome, ci, pos, text, st)
                            if L >= 75 and cls != "Hend" and st[1] == "+":
                                for nm in sorted({v, v + 1} - {0}):
                                    _rd(out, "Hover" if nm == v + 1 else cls, genome, ci, pos, text, st, subs=tuple(range(L - nm, L)))
    return out
