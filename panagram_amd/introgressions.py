"""The calling step of the reference's introgression caller (``panagram intros``: panagram/introgressions/
call_introgressions.py, introgression_runner.py), on k-mer similarity binned on the GPU.

* ``Genome.kmer_similarity_bins`` (index.py) gives each chromosome's binned frame — ``bitmap_to_bins`` of the reference —
  from the bitmap inflated into HBM and binned by k_bin_colsums.  Each anchor's frames are computed ONCE and serve its genome
  similarities and every chromosome, threshold and comparison group (the reference recomputes them per worker).
* This module restates the rest on those frames: genome similarities (per-genome trimmed mean over every bin), the
  preprocessing (``round(2)``, the ``--gnm`` shift, ``--edg`` tapering, ``--sft`` smoothing), 2-way / 3-way / ``--urf``
  thresholds, ``merged`` calls and the BED records, written as the reference lays them out
  (``<out>/<out.name>_<thr>/raw/<anchor>_<chr>_<grp>.bed``) so that its postprocess and score scripts read them.
* ``main`` is the CLI: ``intros call`` with the flags of call_introgressions.py, ``intros <config.yaml> [--sweep]`` with the
  ``general`` / ``calling`` sections of introgression_runner.py's config.  Postprocessing (liftover), scoring, simulation,
  heatmaps (``--vis``) and UMAP are not provided.
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import warnings
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import pandas as pd

# introgression_runner.py: the thresholds of --sweep, 2-way (cmp == [REF]) and 3-way
SWEEP_2WAY = [0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
SWEEP_3WAY = [0.0, 0.04, 0.08, 0.12, 0.16, 0.2, 0.24, 0.28, 0.32, 0.36, 0.4, 0.44, 0.48, 0.52, 0.56, 0.6, 0.64, 0.68]


# ---------------------------------------------------------------------------
# the calling semantics on binned frames (rows: genomes, columns: bin starts)
# ---------------------------------------------------------------------------
def trimmed_mean(row: pd.Series, trim_std: float) -> float:
    """the row's mean over the values within ``trim_std`` standard deviations (ddof 1) of its mean; -1: the plain mean"""
    mean, std = row.mean(), row.std()
    if trim_std == -1:
        return mean
    return row[(row >= mean - trim_std * std) & (row <= mean + trim_std * std)].mean()


def genome_similarities(frames: Sequence[pd.DataFrame], trim_std: float) -> pd.Series:
    """per genome, the trimmed mean of its similarity over every bin of every chromosome"""
    return pd.concat(list(frames), axis=1).apply(trimmed_mean, trim_std=trim_std, axis=1)


def edge_taper(df: pd.DataFrame, intensity: float = 0.1) -> pd.DataFrame:
    """``--edg``: every row times 1 + intensity * exp(-4 x^2) over x in [-1, 1] across the bins, clipped to [0, 1]; every
    value below 1 then lowered by 0.2 and clipped again"""
    x = np.linspace(-1, 1, df.shape[1])
    window = np.exp(-4 * x ** 2)
    boost = intensity * (window / window.max()) if df.shape[1] else window
    out = (df * (1 + boost)).clip(0, 1)
    out = out.where(out == 1, out - 0.2)
    return out.clip(0, 1)


def smooth(df: pd.DataFrame, kind: str, size: int) -> pd.DataFrame:
    """``--sft mean|median``: scipy's uniform_filter1d / median_filter of ``size`` bins along each row, default modes"""
    from scipy.ndimage import median_filter, uniform_filter1d
    if kind not in ("mean", "median"):
        raise ValueError("Invalid smoothing filter selected. Can be mean, median, or None.")
    f = (lambda v: uniform_filter1d(v, size=size)) if kind == "mean" else (lambda v: median_filter(v, size=size))
    vals = np.stack([f(df.iloc[i].to_numpy()) for i in range(df.shape[0])]) if df.shape[0] else df.to_numpy()
    return pd.DataFrame(vals, index=df.index, columns=df.columns)


def preprocess(frame: pd.DataFrame, sims: Optional[pd.Series], gnm: Optional[float], sft: Optional[str], ssz: int,
               edg: bool) -> pd.DataFrame:
    """round(2); with ``sims``, every value <= 0.98 moved by gnm - sims[genome] (gnm -1: the largest similarity other than
    1), then clipped to [0, 1]; then ``--edg``; then ``--sft``"""
    out = frame.round(2)
    if sims is not None:
        if gnm == -1:
            gnm = sims[sims != 1].max()
        delta = (gnm - sims).reindex(out.index).to_numpy(np.float64)
        v = out.to_numpy(np.float64, copy=True)
        m = v <= 0.98
        v[m] += np.broadcast_to(delta[:, None], v.shape)[m]
        out = pd.DataFrame(np.clip(v, 0, 1), index=out.index, columns=out.columns)
    if edg:
        out = edge_taper(out)
    if sft:
        out = smooth(out, sft, ssz)
    return out


def call_group(frame: pd.DataFrame, groups: pd.Series, anchor: str, comp: str, thr: float) -> pd.Series:
    """per bin, 1 where ``anchor`` looks introgressed against ``comp``.  2-way (comp REF): the REF group's largest
    similarity is below thr; 3-way: the REF group's mean is below 0.95 and the comparison group's largest similarity at
    least that mean + thr (the anchor's own group does not enter the call)"""
    grp = groups.reindex(frame.index)
    comp_sim = frame[grp == comp].max(axis=0)
    if comp == "REF":
        call = comp_sim < thr
    else:
        ref_sim = frame[grp == "REF"].mean(axis=0)
        call = (ref_sim < 0.95) & (comp_sim >= ref_sim + thr)
    return call.astype(int)


def call_simple(frame: pd.DataFrame, anchor: str, thr: float) -> pd.Series:
    """``--urf``: in the reference's view, 1 where the anchor's similarity is below thr"""
    return (frame.loc[anchor] < thr).astype(int)


def bed_records(calls: pd.Series, bin_size: int, chrom: str, name: str) -> List[tuple]:
    """runs of called bins whose starts lie bin_size apart -> (chr, start, start + n * bin_size - 1, <name>_intro)"""
    starts = np.asarray(calls.index[calls.to_numpy() > 0], np.int64)
    out = []
    i = 0
    while i < len(starts):
        j = i
        while j + 1 < len(starts) and starts[j + 1] == starts[j] + bin_size:
            j += 1
        out.append((chrom, int(starts[i]), int(starts[i]) + (j - i + 1) * bin_size - 1, f"{name}_intro"))
        i = j + 1
    return out


def write_bed(path: Path, records: List[tuple]) -> None:
    with open(path, "w") as f:
        f.writelines(f"{c}\t{s}\t{e}\t{n}\n" for c, s, e, n in records)


def threshold_dir(out: Path, thr: float) -> Path:
    return out / f"{out.name}_{thr}"


# ---------------------------------------------------------------------------
# options and their checks (call_introgressions.py: main)
# ---------------------------------------------------------------------------
def call_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="panagram_amd intros call", description="Introgression highlighter tool.")
    ap.add_argument("--threads", type=int, default=1, help="accepted for compatibility: the binning runs on the GPU")
    ap.add_argument("--stp", type=int, default=100, help="bitmap kmer step size")
    ap.add_argument("--bin", type=int, default=1000000, help="size of bitmap bin in bases")
    ap.add_argument("--gnm", type=float, help="target mean kmer similarity to normalize each genome to (-1: max average kmer sim.)")
    ap.add_argument("--trm", type=float, default=3.0, help="standard deviations of the trimmed mean normalization (-1: untrimmed)")
    ap.add_argument("--sft", type=str, help="filter type for smoothing (mean or median)")
    ap.add_argument("--ssz", type=int, default=5, help="filter size for smoothing")
    ap.add_argument("--edg", action="store_true", help="perform edge tapered normalization on binned bitmap")
    ap.add_argument("--rmf", action="store_true", help="remove fixed kmers from bitmap")
    ap.add_argument("--rmu", nargs="+", help="remove unique kmers from given genomes; use 'true' to apply to all anchors")
    ap.add_argument("--ogrp", nargs="+", help="group(s) to use as outgroup when using --rmu")
    ap.add_argument("--vis", action="store_true", help="not provided: ignored with a warning")
    ap.add_argument("--urf", action="store_true", help="when using REF as comp group, use the reference's view")
    ap.add_argument("--ref", type=str, help="name of reference genome if using --rmu or --urf")
    ap.add_argument("--anc", nargs="+", help="name of anchor(s) to mark introgressions for")
    ap.add_argument("--grp", nargs="+", help="if --anc is not defined, groups in the tsv to mark introgressions for")
    ap.add_argument("--chr", nargs="+", help="chromosome(s) to mark introgressions for (default: all)")
    ap.add_argument("--cmp", nargs="+", required=True, help="group(s) to compare against anchor(s)")
    ap.add_argument("--thr", type=float, nargs="+", help="threshold(s) for 2-way or 3-way introgression calling")
    ap.add_argument("--idx", type=str, required=True, help="path to Panagram index folder")
    ap.add_argument("--tsv", type=str, required=True, help="path to accession group TSV file")
    ap.add_argument("--out", type=str, required=True, help="path to folder to save all outputs")
    ap.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    return ap


def read_groups(tsv) -> pd.Series:
    tsv = Path(tsv)
    if not tsv.is_file():
        raise ValueError(f"TSV file {tsv} not found. Check --tsv path.")
    groups = pd.read_csv(tsv, sep="\t", index_col=0)
    groups.index = groups.index.astype(str)
    if groups["group"].astype("string").str.contains("_", na=False).any():
        raise ValueError("Group names cannot contain underscores ('_').")
    return groups["group"]


def plan(a: argparse.Namespace, groups: pd.Series) -> dict:
    """the checked options of one calling run: anchors, comparison groups, --rmu accessions and their keep mask"""
    if not a.thr:
        raise ValueError("At least one threshold must be provided with --thr.")
    if a.sft not in (None, "mean", "median"):
        raise ValueError("Invalid smoothing filter selected. Can be mean, median, or None.")
    anchors = a.anc
    if anchors is None:
        if a.grp is None:
            raise ValueError("No anchor selected. Use either --anc or --grp to specify anchors.")
        anchors = list(groups[groups.isin(a.grp)].index)
    elif a.grp is not None:
        raise ValueError("Cannot use both --anc and --grp. Use one or the other.")
    rmu, outgroup = a.rmu, []
    if rmu is not None:
        if a.ref is None:
            raise ValueError("Reference genome must be provided using --ref when using --rmu.")
        if len(rmu) == 1 and rmu[0] == "true":
            rmu = list(anchors)
        if a.ogrp is None:
            raise ValueError("Outgroup groups must be provided using --ogrp when using --rmu.")
        outgroup = list(groups[groups.isin(a.ogrp)].index)
        if "REF" in outgroup:
            raise ValueError("REF cannot be used as an outgroup accession. Please remove REF from the groups specified in --ogrp.")
        if any(acc in outgroup for acc in rmu):
            raise ValueError("Accessions specified in --rmu cannot be in the outgroup. Please remove any accessions specified "
                             "in --rmu from the groups specified in --ogrp.")
    comp = list(dict.fromkeys(a.cmp))
    if "REF" in comp and comp != ["REF"]:
        raise ValueError("Error: REF must be the only comparison group specified so that a 2-way comparison can be run.")
    if a.urf and comp != ["REF"]:
        raise ValueError("REF must be the only comparison group specified with --cmp if using --urf.")
    for anc in anchors:
        if anc not in groups.index:
            raise ValueError(f"anchor {anc} is not listed in the group TSV")
    return dict(anchors=list(anchors), comp=comp, rmu=rmu or [], keep=outgroup + [a.ref] if rmu else None,
                thresholds=[float(t) for t in a.thr])


def _genome(idx, name: str):
    if name not in idx.genomes:
        raise ValueError(f"genome {name} is not in the index")
    g = idx[name]
    if not g.anchored or not os.path.exists(g.chrs_fname) or not os.path.exists(g.bitmap_gz_fname(1)):
        raise ValueError(f"genome {name} has no bitmaps in the index (it is not an anchored genome)")
    if g.chrs is None:
        g.load_chrs()
    return g


def run_call(a: argparse.Namespace, idx=None, log=print) -> Path:
    """``intros call``: raw BED files of every anchor, chromosome, threshold and comparison group under ``a.out``"""
    if a.vis:
        warnings.warn("--vis: heatmaps are not provided; ignored")
    groups = read_groups(a.tsv)
    p = plan(a, groups)
    out = Path(a.out)
    own = idx is None
    if own:
        from .index import Index
        if not Path(a.idx).is_dir():
            raise ValueError(f"Index directory {a.idx} not found. Check --idx path.")
        idx = Index(str(a.idx), mode="r", device=a.device)
    try:
        for anc in p["anchors"]:  # every anchor's genome is checked before any work
            _genome(idx, anc)
        if a.urf:
            if a.ref is None:
                raise ValueError("Reference genome must be provided using --ref when using --urf.")
            _genome(idx, a.ref)
        frames_of: Dict[tuple, Dict[str, pd.DataFrame]] = {}
        sims_of: Dict[tuple, Optional[pd.Series]] = {}

        def binned(name: str, keep, chroms: Optional[List[str]]):
            """the genome's frames and genome similarities for one keep mask, computed once"""
            key = (name, tuple(keep) if keep else None)
            g = idx[name]
            want = list(g.chrs.index) if a.gnm or chroms is None else list(dict.fromkeys(chroms))
            have = frames_of.setdefault(key, {})
            todo = [c for c in want if c not in have]
            if todo:
                missing = [c for c in todo if c not in g.chrs.index]
                if missing:
                    raise ValueError(f"genome {name} has no chromosome {missing[0]}")
                have.update(g.kmer_similarity_bins(todo, step=a.stp, bin_size=a.bin, omit_fixed=a.rmf, keep=keep))
            if key not in sims_of:
                sims_of[key] = genome_similarities([have[c] for c in g.chrs.index], a.trm) if a.gnm else None
            return have, sims_of[key]

        for anc in p["anchors"]:
            log("Now running introgression analysis for", anc)
            anchor_group = groups.loc[anc]
            comps = [c for c in p["comp"] if c != anchor_group]
            if not comps:
                log(f"Skipping {anc}: no comparison groups left after removing {anchor_group}.")
                continue
            rmu = anc in p["rmu"]
            urf = a.urf and not rmu
            if a.urf and rmu:
                log("Note that this accession will output REFA files to allow rmu to run.")
            chroms = list(a.chr) if a.chr else list(idx[anc].chrs.index)
            src = a.ref if urf else anc
            frames, sims = binned(src, p["keep"] if rmu else None, chroms)
            for chrom in chroms:
                if chrom not in frames:
                    raise ValueError(f"genome {src} has no chromosome {chrom}")
                fr = preprocess(frames[chrom], sims, a.gnm, a.sft, a.ssz, a.edg)
                for thr in p["thresholds"]:
                    raw = threshold_dir(out, thr) / "raw"
                    raw.mkdir(parents=True, exist_ok=True)
                    merged = None
                    for comp in comps:
                        calls = call_simple(fr, anc, thr) if urf else call_group(fr, groups, anc, comp, thr)
                        name = "REFA" if comp == "REF" and not urf else comp
                        write_bed(raw / f"{anc}_{chrom}_{name}.bed", bed_records(calls, a.bin, chrom, name))
                        if len(comps) > 1:
                            merged = calls if merged is None else merged + calls
                    if merged is not None:
                        write_bed(raw / f"{anc}_{chrom}_merged.bed", bed_records(merged, a.bin, chrom, "merged"))
        log("Done.")
    finally:
        if own:
            idx.close()
    return out


# ---------------------------------------------------------------------------
# intros <config.yaml> [--sweep] (introgression_runner.py)
# ---------------------------------------------------------------------------
def config_argv(config_path, sweep: bool = False) -> List[str]:
    """the ``intros call`` argument list of a runner config (its ``general`` and ``calling`` sections).  Raises before any
    work when the config asks for postprocessing or scoring, which are not provided; ``vis`` is ignored with a warning.
    An empty list: the config does not run the calling step."""
    import yaml
    config_path = Path(config_path)
    if not config_path.is_file():
        raise ValueError(f"Config file {config_path} does not exist.")
    with config_path.open() as f:
        cfg = yaml.safe_load(f) or {}
    for sec in ("postprocessing", "scoring"):
        if (cfg.get(sec) or {}).get("run"):
            raise ValueError(f"{sec}.run is true: the {sec} step is not provided (only the calling step is); set it to false")
    general, calling = cfg.get("general") or {}, cfg.get("calling") or {}
    for key in ("output_dir", "index_dir", "tsv", "bin"):
        if general.get(key) is None:
            raise ValueError(f"{config_path}: general.{key} is required")
    if not calling.get("run"):
        return []
    if calling.get("vis"):
        warnings.warn("calling.vis: heatmaps are not provided; ignored")
    cmp = [str(c) for c in calling.get("cmp") or []]
    thr = calling.get("thr") or []
    if sweep:
        thr = SWEEP_2WAY if cmp == ["REF"] else SWEEP_3WAY
    thr = [float(t) for t in thr]

    def names(v):
        return [str(x) for x in (v if isinstance(v, (list, tuple)) else [v])]
    argv = ["--out", str(Path(general["output_dir"]).resolve()), "--idx", str(Path(general["index_dir"]).resolve()),
            "--tsv", str(Path(general["tsv"]).resolve()), "--bin", str(general["bin"]), "--stp", str(calling.get("stp", 100))]
    if calling.get("grp"):
        argv += ["--grp"] + names(calling["grp"])
    if calling.get("anc"):
        argv += ["--anc"] + names(calling["anc"])
    if calling.get("chr"):
        argv += ["--chr"] + names(calling["chr"])
    if cmp:
        argv += ["--cmp"] + cmp
    for key in ("gnm", "trm", "sft", "ssz"):
        if calling.get(key) is not None:
            argv += [f"--{key}", str(calling[key])]
    if calling.get("urf"):
        argv.append("--urf")
    rmu = calling.get("rmu")
    if rmu is True:
        argv += ["--rmu", "true"]
    elif rmu:
        argv += ["--rmu"] + names(rmu)
    if calling.get("ogrp"):
        argv += ["--ogrp"] + names(calling["ogrp"])
    if general.get("ref") is not None:
        argv += ["--ref", str(general["ref"])]
    if calling.get("rmf"):
        argv.append("--rmf")
    if calling.get("edg"):
        argv.append("--edg")
    if thr:
        argv += ["--thr"] + [str(t) for t in thr]
    return argv


def run_config(config_path, sweep: bool = False, device: Optional[int] = None, log=print) -> Optional[Path]:
    argv = config_argv(config_path, sweep)
    if not argv:
        log("calling.run is false: nothing to do.")
        return None
    if device is not None:
        argv += ["--device", str(device)]
    a = call_parser().parse_args(argv)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    shutil.copy(config_path, out / "intro_config.yaml")
    run_call(a, log=log)
    log("Introgressions analysis complete.")
    return out


def main(argv: Optional[Sequence[str]] = None) -> int:
    """``intros call [flags of call_introgressions.py]`` or ``intros <config.yaml> [--sweep] [--device D]``"""
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print("usage: panagram_amd intros call --idx IDX --tsv TSV --out OUT --cmp GRP [...] --thr THR [...]\n"
              "       panagram_amd intros <config.yaml> [--sweep] [--device D]")
        return 0
    if argv[0] == "call":
        run_call(call_parser().parse_args(argv[1:]))
        return 0
    ap = argparse.ArgumentParser(prog="panagram_amd intros")
    ap.add_argument("config")
    ap.add_argument("--sweep", action="store_true", help="run the preset list of thresholds")
    ap.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    c = ap.parse_args(argv)
    run_config(c.config, c.sweep, c.device)
    return 0
