"""A restatement, for the tests, of the introgression caller's calling rules (panagram/introgressions/
call_introgressions.py) in plain pandas on the rows of a bitmap: what `intros` must reproduce.  Written from the rules,
not copied; the product (panagram_amd/introgressions.py, Genome.kmer_similarity_bins) shares no code with it."""
import gzip

import numpy as np
import pandas as pd
from scipy.ndimage import median_filter, uniform_filter1d


def query_rows(gz_path, nbytes, row0, nrows, stride, ngenomes):
    """rows [row0, row0 + nrows) of a bitmap.<s>.gz payload, every stride-th, as 0/1 columns"""
    raw = np.frombuffer(gzip.decompress(open(gz_path, "rb").read()), np.uint8).reshape(-1, nbytes)
    pac = raw[row0:row0 + nrows][::stride]
    return np.unpackbits(pac, bitorder="little", axis=1)[:, :ngenomes]


def query_frame(genome_dir, names, chrs, steps, chrom, step):
    """genome.query(chrom, 0, size, step) as the reference builds it"""
    n = len(names)
    nb = (n + 7) // 8
    bstep = max(s for s in steps if step % s == 0)
    sizes = chrs["size"].astype(np.int64)
    per = -(-sizes // bstep)
    row0 = int(per.cumsum().shift(fill_value=0).loc[chrom])
    size = int(sizes.loc[chrom])
    nrows = (size - 1) // bstep + 1 if size else 0
    bits = query_rows(f"{genome_dir}/bitmap.{bstep}.gz", nb, row0, nrows, step // bstep, n)
    return pd.DataFrame(bits, index=pd.RangeIndex(0, size, step)[:len(bits)], columns=names)


def bitmap_to_bins(bitmap, binlen, omit_fixed=False, keep_cols=None):
    """rows -> bins (by position // binlen) -> per-genome sums -> divided by each bin's largest sum"""
    df = bitmap.set_index(bitmap.index // binlen)
    if keep_cols is not None:
        none = df[keep_cols].sum(axis=1) == 0
        df.loc[none, keep_cols] = 1
    bins = df.index.unique()
    if omit_fixed:
        df = df.loc[~(df == 1).all(axis=1)]
    sums = df.groupby(level=0).sum().reindex(bins, fill_value=1)
    sums = sums.set_index(sums.index * binlen).T
    return sums.div(sums.max(axis=0), axis=1)


def trimmed_mean(row, t):
    m, sd = row.mean(), row.std()
    if t == -1:
        return m
    return row[(row >= m - t * sd) & (row <= m + t * sd)].mean()


def similarities(frames, t):
    return pd.concat(frames, axis=1).apply(trimmed_mean, axis=1, args=(t,))


def preprocess(df, sims, gnm, sft, ssz, edg):
    df = df.copy().round(2)
    if sims is not None:
        if gnm == -1:
            gnm = sims[sims != 1].max()
        shift = gnm - sims
        for g in df.index:
            r = df.loc[g].copy()
            low = r <= 0.98
            r[low] = r[low] + shift[g]
            df.loc[g] = r.clip(0, 1)
    if edg:
        x = np.linspace(-1, 1, df.shape[1])
        w = np.exp(-4 * x ** 2)
        boost = 0.1 * w / w.max()
        for g in df.index:
            df.loc[g] = df.loc[g] * (1 + boost)
        df = df.clip(0, 1)
        df = df.where(df == 1, df - 0.2).clip(0, 1)
    if sft:
        f = (lambda v: uniform_filter1d(v, size=ssz)) if sft == "mean" else (lambda v: median_filter(v, size=ssz))
        df = df.apply(lambda r: pd.Series(f(r.values), index=r.index), axis=1)
    return df


def calls_3way_or_2way(df, groups, comp, thr):
    g = pd.Series([groups.get(n) for n in df.index], index=df.index)
    comp_max = df[g == comp].max(axis=0)
    if comp == "REF":
        return (comp_max < thr).astype(int)
    ref_mean = df[g == "REF"].mean(axis=0)
    return ((ref_mean < 0.95) & (comp_max >= ref_mean + thr)).astype(int)


def bed_text(calls, binlen, chrom, name):
    """adjacent called bins -> one record, end = start + n * binlen - 1"""
    lines, run = [], None
    for start, v in calls.items():
        if v <= 0:
            continue
        if run and start == run[1]:
            run = (run[0], start + binlen, run[2] + 1)
        else:
            if run:
                lines.append((run[0], run[2]))
            run = (start, start + binlen, 1)
    if run:
        lines.append((run[0], run[2]))
    return "".join(f"{chrom}\t{s}\t{s + n * binlen - 1}\t{name}_intro\n" for s, n in lines)
