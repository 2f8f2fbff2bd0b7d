"""CLI surface kept from the reference (`panagram index <samples.tsv> -k K [-o prefix] [-c cores]
[--prepare]`, panagram/__main__.py:154-194, index.py:90-123) plus the process-level seam of
cpp/run_anchor (`run_anchor <ngenomes> <root> [<name> <fasta>]...`), and what the reference only does inside its viewer:
`tree <index_dir> <genome> <chrom> [start] [end] [step]` prints the Newick tree of the genomes over a region;
`umaps <index_dir> [genome ...]` writes chrom_umaps.csv and genome_umap.csv (index.py:1107-1156) for an existing index; and
`find <index_dir> <genome> [chrom] [start] [end] [step] --have A,B --lack C,D` lists the runs of positions whose k-mers the
`--have` genomes hold and the `--lack` genomes do not (the query scripts/query_index.py's "custom" branch sketches);
`patterns <index_dir> <genome> [chrom] [start] [end] [step] [--genomes A,B,...]` lists the presence/absence patterns that occur in
a region's rows with the rows each holds (query_bitmap + value_counts(), reduced on the GPU);
`gaps <index_dir> <genome> [chrom] [start] [end] [--genomes A,B,...]` lists, per genome, the runs of positions whose k-mers it lacks
with the kind of difference their length suggests (query_bitmap + a per-column np.diff, reduced on the GPU);
`pangenome <index_dir> [--matrix FILE] [--occupancy FILE]` prints every sample's distinct, private, core and shell k-mers, counted
on the GPU in one pass over the table of all samples' k-mers (`index --kmer_stats` writes the matrix and the occupancy table with
the index; `dist <index_dir> --exact` writes genome_dist.tsv from the exact Jaccard index at the index's k); and
`synteny <index_dir> <A> <B> [--chroms-a X,Y] [--chroms-b ...] [-k K] [--min-len N]` lists the maximal collinear runs of k-mers that
occur exactly once in genome A and exactly once in genome B, with their place and strand in B, found on the GPU from the two
genomes' sequences (the lines of a dot plot; the reference has nothing that says WHERE in B a k-mer lies);
`synteny <index_dir> <A> <B> --blocks [--min-run N] [--max-gap G] [--max-shift S] [--paf]` chains those runs on the GPU into blocks
that bridge substitutions and small insertions and deletions — a few thousand lines where the runs are a million — with the runs
and the shifted links of each, or as PAF lines for the tools that draw dot plots; the runs never leave the GPU;
`synteny <index_dir> <A> <B> --variants [--vcf] [--min-run N] [--max-gap G] [--max-shift S] [--summary FILE]` says what differs inside
those blocks: every link of every block is classified and compared base by base on the GPU, and the SNPs, insertions and deletions of
B against A come out with their place on both genomes and both alleles — as a table, or as a VCF of B against A; and
`search <index_dir> <queries.fa> [--genomes A,B] [--min-frac F] [--by kmers|bases] [--matrix FILE] [--summary FILE]` says which genomes
carry each query sequence — a gene, a marker, a contig that is NOT in the index — and how completely: the query's k-mers are probed
against the table of every sample's k-mers and their rows reduced per query and genome on the GPU; and
`copies <index_dir> [targets.fa] [--genes GENOME] [--genomes A,B] [-k K] [--matrix FILE] [--summary FILE] [--track FILE]` says how MANY
copies of each target sequence — the records of a FASTA, or the annotated genes of a genome — the genomes' assemblies hold: the
targets' k-mers go into a count table, every genome is streamed through it, and the depths along each target are reduced to a
histogram and its median on the GPU; and
`locate <index_dir> [queries.fa] [--genes GENOME] [--genomes A,B] [-k K] [--min-run N] [--max-gap G] [--max-shift S] [--min-kmers N]
[--min-frac F] [--paf] [--matrix FILE] [--summary FILE]` says WHERE each query lies in every genome — chromosome, start, end, strand,
every copy: the queries' k-mers go into a position table, every genome's assembly is streamed through it, and the collinear runs of
its hits are chained into loci on the GPU; only the loci leave it; and
`screen <index_dir> <sample.fq|sample.fa> [more ...] [--min-count N] [--genomes A,B] [--occupancy FILE] [--summary FILE]` says which
of the indexed genomes a sample from outside the index holds and how much of each: the reads, or an assembly, are streamed once
through the table of every sample's k-mers and counted per k-mer, and one pass over the table joins the counts with the presence
masks on the GPU; and
`novel <index_dir> <sample.fq|sample.fa> [more ...] [--min-count N] [--spectrum FILE] [--kmers FILE] [--regions FILE] [--min-bases B]
[--unitigs FILE] [--min-unitig-bases B] [--clean [--tip-kmers T] [--bubble-kmers B] [--clean-ratio R] [--clean-rounds N]]
[--summary FILE]` says the reverse: the distinct k-mers of the sample that NO indexed genome
holds, their depth spectrum, for an assembly where they lie, and with --unitigs the novel sequences themselves, the solid k-mers
compacted into unitigs, with --clean after error tips were clipped and bubbles popped — the sample's windows that miss the table are counted in a key table of their own that grows on the GPU; and
`add <index_dir> <new_samples.tsv>` appends samples to a finished index without re-anchoring it: every anchor already there is probed
against the new samples' k-mers alone, its rows come back from bitmap.1.gz, and one kernel pass writes the wider rows; new anchors are
anchored the ordinary way, and the tree is staged and renamed at the end, samples.tsv last; and
`subset <index_dir> -o <out_dir> (--keep A,B,... | --drop C,D,...) [--anchors A,B] [--no-sequence-files]` writes an index of the
chosen samples into a new directory: the kept anchors' rows come back from bitmap.1.gz and one kernel pass takes the kept columns
out of them, in the order asked for; no sequence is read; and
`genotype <index_dir> <A> <B> <sample.fq|sample.fa> [more ...] [--chroms-a X,Y] [--chroms-b X,Y] [-k K] [--min-run N] [--max-gap G]
[--max-shift S] [--min-count C] [--min-frac F] [--vcf] [--sample NAME] [--summary FILE]` joins the two sides: at every variant of B
against A that `synteny --variants` calls, which allele does a third, unassembled sample carry?  The k-mers that span either allele go
into a count table on the GPU, the whole assemblies of A and B and the sample's reads are streamed through it, and per variant and
allele the k-mers that occur once in the allele's genome and never in the other are counted with those the sample holds: `0/0`, `0/1`,
`1/1` or `./.`, as a table or as a VCF with a sample column.  Limits: variants closer than k share windows, `--min-count` is the only
error filter, depths are not modelled (`0/1` is also what a mixture gives), four-line FASTQ, k <= 32, 2^30 keys."""
import argparse
import os
import sys


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == "intros":  # (its own two forms: `intros call ...` and `intros <config.yaml>`)
        from . import introgressions
        return introgressions.main(argv[1:])
    ap = argparse.ArgumentParser(prog="panagram_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    ix = sub.add_parser("index", help="Anchor k-mer bitvectors to reference FASTA files to create pan-kmer bitmap")
    ix.add_argument("input", metavar="config_file")
    ix.add_argument("-o", "--prefix", default=None)
    ix.add_argument("-k", type=int, default=21)
    ix.add_argument("-c", "--cores", type=int, default=1)
    ix.add_argument("-p", "--prepare", action="store_true")
    ix.add_argument("--anchor_genomes", nargs="*", default=None)
    # one process per GPU under torchrun: LOCAL_RANK picks the GPU, RANK / WORLD_SIZE the anchor genomes
    ix.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    ix.add_argument("--export_kmc", action="store_true", help="also write kmc/bitvec{i} (KMC1 layout)")
    ix.add_argument("--kmc.use_existing", dest="use_existing", action="store_true")
    ix.add_argument("--genome_dist", action="store_true", help="also write genome_dist.tsv (MinHash distances, for panagram view)")
    ix.add_argument("--annotate", action="store_true", help="also write the gene / annotation tracks of annotated anchor genomes")
    ix.add_argument("--umaps", action="store_true", help="also write chrom_umaps.csv and genome_umap.csv of the anchor genomes")
    ix.add_argument("--kmer_stats", action="store_true", help="also write kmer_shared.tsv and kmer_occupancy.tsv: the distinct k-mers "
                    "every pair of samples shares and the k-mers held by n samples, counted on the GPU off the table of all samples")
    ds = sub.add_parser("dist", help="write genome_dist.tsv of an existing index (MinHash sketches on the GPU)")
    ds.add_argument("index_dir")
    ds.add_argument("--exact", action="store_true", help="the exact Jaccard index of the samples' distinct k-mers at the index's k "
                    "(counted on the GPU off the k-mer table) in place of the MinHash estimate at k = 21; the p-value column reads 0")
    ds.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    pg = sub.add_parser("pangenome", help="distinct, private, core and shell k-mers of every sample of an index, counted on the GPU "
                                          "in one pass over the k-mer table: tab-separated name kmers private core shell")
    pg.add_argument("index_dir")
    pg.add_argument("--matrix", metavar="FILE", default=None, help="also write the shared distinct k-mers of every pair as a tab-separated table")
    pg.add_argument("--occupancy", metavar="FILE", default=None, help="also write n kmers: the distinct k-mers held by n of the samples")
    pg.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    an = sub.add_parser("annotate", help="(Re-)annotate an existing anchored genome using a GFF file")
    an.add_argument("index_dir")
    an.add_argument("genome")
    an.add_argument("gff_file")
    an.add_argument("--nogene", action="store_true")
    an.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    tr = sub.add_parser("tree", help="Newick tree of the genomes over a region of an anchored genome, from pair counts of its "
                                     "bitmap rows reduced on the GPU")
    tr.add_argument("index_dir")
    tr.add_argument("genome")
    tr.add_argument("chrom", nargs="?", default=None)
    tr.add_argument("start", nargs="?", type=int, default=None)
    tr.add_argument("end", nargs="?", type=int, default=None)
    tr.add_argument("step", nargs="?", type=int, default=None, help="default: the index's low-resolution step")
    tr.add_argument("--whole", action="store_true", help="the whole genome in place of a chromosome")
    tr.add_argument("--matrix", metavar="FILE", default=None, help="also write the pair counts as a tab-separated table")
    tr.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    fd = sub.add_parser("find", help="runs of positions whose k-mers the --have genomes hold and the --lack genomes lack, found "
                                     "in the bitmap rows on the GPU: tab-separated chrom start end rows")
    fd.add_argument("index_dir")
    fd.add_argument("genome")
    fd.add_argument("chrom", nargs="?", default=None)
    fd.add_argument("start", nargs="?", type=int, default=None)
    fd.add_argument("end", nargs="?", type=int, default=None)
    fd.add_argument("step", nargs="?", type=int, default=1)
    fd.add_argument("--have", default="", metavar="A,B", help="genomes that hold the k-mer")
    fd.add_argument("--lack", default="", metavar="C,D", help="genomes that do not")
    fd.add_argument("--min-have", type=int, default=None, metavar="N", help="at least N of --have (default: all of them)")
    fd.add_argument("--max-lack", type=int, default=0, metavar="N", help="at most N of --lack (default: 0)")
    fd.add_argument("--min-len", type=int, default=1, metavar="N", help="drop runs of fewer than N rows")
    fd.add_argument("--max-gap", type=int, default=0, metavar="N", help="first merge runs at most N non-matching rows apart")
    fd.add_argument("--density", type=int, default=None, metavar="BIN_SIZE",
                    help="write chrom start matched rows per bin of BIN_SIZE positions instead")
    fd.add_argument("--whole", action="store_true", help="the whole genome in place of a chromosome")
    fd.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    fd.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    pt = sub.add_parser("patterns", help="the presence/absence patterns that occur in a region's bitmap rows and the rows each "
                                         "holds, counted on the GPU: tab-separated pattern n rows frac genomes")
    pt.add_argument("index_dir")
    pt.add_argument("genome")
    pt.add_argument("chrom", nargs="?", default=None)
    pt.add_argument("start", nargs="?", type=int, default=None)
    pt.add_argument("end", nargs="?", type=int, default=None)
    pt.add_argument("step", nargs="?", type=int, default=1)
    pt.add_argument("--genomes", default="", metavar="A,B", help="the genomes of a pattern, at most 64 (default: all of them)")
    pt.add_argument("--top", type=int, default=None, metavar="K", help="only the K patterns with the most rows")
    pt.add_argument("--min-rows", type=int, default=1, metavar="N", help="drop patterns of fewer than N rows")
    pt.add_argument("--occupancy", action="store_true", help="write n rows instead: the rows held by n of the genomes, n = 0..m")
    pt.add_argument("--whole", action="store_true", help="the whole genome in place of a chromosome")
    pt.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    pt.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    gp = sub.add_parser("gaps", help="per genome, the runs of positions whose k-mers it lacks — a substitution clears k rows, an "
                                     "insertion k - 1, a deletion of d bases k - 1 + d — counted in the bitmap rows on the GPU: "
                                     "tab-separated chrom start end genome rows class site")
    gp.add_argument("index_dir")
    gp.add_argument("genome")
    gp.add_argument("chrom", nargs="?", default=None)
    gp.add_argument("start", nargs="?", type=int, default=None)
    gp.add_argument("end", nargs="?", type=int, default=None)
    gp.add_argument("--genomes", default="", metavar="A,B", help="the genomes to follow (default: all of them)")
    gp.add_argument("--min-len", type=int, default=None, metavar="N", help="drop runs of fewer than N rows (default: k - 1)")
    gp.add_argument("--max-len", type=int, default=0, metavar="N", help="drop runs of more than N rows (default 0: none)")
    gp.add_argument("--maxlen", type=int, default=None, metavar="N", help="the spectrum's last bin: runs of N rows and more (default: 4 k)")
    gp.add_argument("--spectrum", metavar="FILE", default=None, help="also write genome rows runs: the closed runs of every length")
    gp.add_argument("--summary", metavar="FILE", default=None, help="also write one line per genome: rows, absent rows, runs by class")
    gp.add_argument("--whole", action="store_true", help="the whole genome in place of a chromosome")
    gp.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    gp.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    sy = sub.add_parser("synteny", help="the maximal collinear runs of k-mers unique in genome A and unique in genome B, found on the "
                                        "GPU from the two genomes' sequences: tab-separated chrA startA endA chrB startB endB strand kmers")
    sy.add_argument("index_dir")
    sy.add_argument("genome_a", metavar="A")
    sy.add_argument("genome_b", metavar="B")
    sy.add_argument("--chroms-a", default="", metavar="X,Y", help="only these chromosomes of A (default: all of them)")
    sy.add_argument("--chroms-b", default="", metavar="X,Y", help="only these chromosomes of B (default: all of them)")
    sy.add_argument("-k", type=int, default=None, help="1 to 32 (default: the index's k)")
    sy.add_argument("--min-len", type=int, default=1, metavar="N", help="drop runs (with --blocks: blocks) of fewer than N k-mers")
    sy.add_argument("--blocks", action="store_true", help="chain the runs on the GPU into blocks that bridge substitutions and small "
                    "insertions and deletions: the same columns, then runs and shifted (the links whose gaps differ on A and B)")
    sy.add_argument("--variants", action="store_true", help="the differences inside the blocks, found on the GPU from the blocks' links: "
                    "chrA posA refLen chrB posB altLen strand class mismatches ref alt, one line per snp, mnp, ins, del or complex "
                    "variant of B against A (alt in A's orientation; - for an empty allele)")
    sy.add_argument("--vcf", action="store_true", help="with --variants: VCF 4.2 lines of B against A in place of the table")
    sy.add_argument("--min-run", type=int, default=None, metavar="N", help="with --blocks or --variants: runs of fewer than N k-mers neither "
                    "join nor break a block (default 1)")
    sy.add_argument("--max-gap", type=int, default=None, metavar="G", help="with --blocks or --variants: a run joins the block of the run before "
                    "it when it starts at most G positions behind that run's last k-mer, on A and on B (default 1000)")
    sy.add_argument("--max-shift", type=int, default=None, metavar="S", help="with --blocks or --variants: ... and the two distances differ by at "
                    "most S: the longest insertion or deletion bridged (default 100)")
    sy.add_argument("--paf", action="store_true", help="with --blocks: PAF lines (query A, target B, matches = k-mers, tags rn:i: "
                    "runs and sh:i: shifted links) in place of the table")
    sy.add_argument("--summary", metavar="FILE", default=None, help="also write chrA chrB strand segments kmers: the segments and shared "
                    "unique k-mers of every pair of chromosomes and strand, then per chromosome of either side, then in all; in front, "
                    "as # lines, per side the positions whose k-mer is unique in that genome and those with a mate; with --variants: class count "
                    "basesA basesB per class of variant, then the links without a difference and all links")
    sy.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    sy.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    ge = sub.add_parser("genotype", help="which allele a sample from outside the index carries at every variant of genome B against genome "
                                         "A: the k-mers that span either allele counted in A, in B and in the sample's reads (or assembly) on "
                                         "the GPU: tab-separated, with a header, chrA posA refLen chrB posB altLen strand class ref alt "
                                         "ref_kmers ref_seen ref_depth alt_kmers alt_seen alt_depth GT flag")
    ge.add_argument("index_dir")
    ge.add_argument("genome_a", metavar="A")
    ge.add_argument("genome_b", metavar="B")
    ge.add_argument("samples", metavar="sample.fq|sample.fa", nargs="+", help="the sample's files: FASTQ (four lines per record) or FASTA, plain or .gz")
    ge.add_argument("--chroms-a", default="", metavar="X,Y", help="variants on these chromosomes of A only (default: all of them)")
    ge.add_argument("--chroms-b", default="", metavar="X,Y", help="variants on these chromosomes of B only (default: all of them)")
    ge.add_argument("-k", type=int, default=None, help="1 to 32 (default: the index's k)")
    ge.add_argument("--min-run", type=int, default=1, metavar="N", help="as synteny --variants (default 1)")
    ge.add_argument("--max-gap", type=int, default=1000, metavar="G", help="as synteny --variants (default 1000)")
    ge.add_argument("--max-shift", type=int, default=100, metavar="S", help="as synteny --variants (default 100)")
    ge.add_argument("--min-count", type=int, default=None, metavar="C",
                    help="the sample holds a k-mer it holds at least C times: the only error filter (default: 2 when a file is FASTQ, else 1)")
    ge.add_argument("--min-frac", type=float, default=0.5, metavar="F",
                    help="an allele is present when the sample holds at least F of its informative k-mers, above 0 to 1 (default 0.5)")
    ge.add_argument("--vcf", action="store_true", help="VCF 4.2 lines of synteny --variants --vcf with one sample column GT:RK:AK in place of the table")
    ge.add_argument("--sample", metavar="NAME", default=None, help="with --vcf: the sample column's name (default: the first sample file's base name)")
    ge.add_argument("--summary", metavar="FILE", default=None, help="also write class GT count; in front, as # lines, reads, windows, hits, "
                    "sites, callable sites, min_count and min_frac")
    ge.add_argument("--batch-bytes", type=int, default=None, metavar="N", help="FASTQ text bytes joined at a time (default 2^28)")
    ge.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    ge.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    se = sub.add_parser("search", help="which genomes carry each query sequence, and how completely: the queries' k-mers probed against "
                                       "the table of every sample's k-mers and reduced per query and genome on the GPU: tab-separated, with "
                                       "a header, query length kmers genome hits frac covered cov_frac runs longest first end")
    se.add_argument("index_dir")
    se.add_argument("queries", metavar="queries.fa", help="FASTA, plain or .gz")
    se.add_argument("--genomes", default="", metavar="A,B", help="the genomes to report (default: all of them)")
    se.add_argument("--min-frac", type=float, default=0.0, metavar="F", help="drop lines whose frac (with --by bases: cov_frac) is below F")
    se.add_argument("--by", choices=["kmers", "bases"], default="kmers", help="what --min-frac, the matrix and the summary's best go by: "
                    "frac = hits / kmers, or cov_frac = covered / length (default: kmers)")
    se.add_argument("--matrix", metavar="FILE", default=None, help="also write the queries x genomes table of frac (--by bases: cov_frac)")
    se.add_argument("--summary", metavar="FILE", default=None, help="also write one line per query: query length kmers all none genomes_hit best best_frac")
    se.add_argument("--batch-bases", type=int, default=None, metavar="N", help="query bases anchored at a time (default 2^26)")
    se.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    se.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    cp = sub.add_parser("copies", help="how many copies of each target sequence the genomes' assemblies hold: the k-mers of every genome "
                                       "counted against the targets' on the GPU, the depth along each target reduced to its median: "
                                       "tab-separated, with a header, target length kmers valid genome present frac copies copies_nz mean max_bin")
    cp.add_argument("index_dir")
    cp.add_argument("targets", metavar="targets.fa", nargs="?", default=None, help="FASTA, plain or .gz (or --genes)")
    cp.add_argument("--genes", metavar="GENOME", default=None, help="the targets are the annotated genes of this genome (in place of targets.fa)")
    cp.add_argument("--genomes", default="", metavar="A,B", help="the genomes to count in (default: all of them)")
    cp.add_argument("-k", type=int, default=None, help="k-mer length, 1 to 32 (default: the index's)")
    cp.add_argument("--matrix", metavar="FILE", default=None, help="also write the targets x genomes table of copies")
    cp.add_argument("--summary", metavar="FILE", default=None, help="also write one line per genome: genome targets 0 1 2 3 4+")
    cp.add_argument("--track", metavar="FILE", default=None, help="also write the runs of equal depth along every target: target genome start end depth")
    cp.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    cp.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    lo = sub.add_parser("locate", help="where each query sequence lies in every genome's assembly, every copy: the genomes streamed through "
                                       "a position table of the queries' k-mers, the runs of hits chained into loci on the GPU: tab-separated, "
                                       "with a header, query genome chrom start end strand qstart qend kmers frac runs shifted")
    lo.add_argument("index_dir")
    lo.add_argument("queries", metavar="queries.fa", nargs="?", default=None, help="FASTA, plain or .gz (or --genes)")
    lo.add_argument("--genes", metavar="GENOME", default=None, help="the queries are the annotated genes of this genome (in place of queries.fa)")
    lo.add_argument("--genomes", default="", metavar="A,B", help="the genomes to look in (default: all of them)")
    lo.add_argument("-k", type=int, default=None, help="k-mer length, 1 to 32 (default: the index's)")
    lo.add_argument("--min-run", type=int, default=1, metavar="N", help="drop runs of fewer than N k-mers before chaining (default 1)")
    lo.add_argument("--max-gap", type=int, default=1000, metavar="G", help="a locus bridges at most G positions on genome and query (default 1000)")
    lo.add_argument("--max-shift", type=int, default=100, metavar="S", help="... whose two distances differ by at most S (default 100)")
    lo.add_argument("--min-kmers", type=int, default=1, metavar="N", help="drop loci of fewer than N matched k-mers (default 1)")
    lo.add_argument("--min-frac", type=float, default=0.0, metavar="F", help="drop loci that hold less than F of the query's unique k-mers")
    lo.add_argument("--paf", action="store_true", help="write PAF lines (query = the query, target = the chromosome; tags rn, sh, gn) in place of the table")
    lo.add_argument("--matrix", metavar="FILE", default=None, help="also write the queries x genomes table of loci")
    lo.add_argument("--summary", metavar="FILE", default=None, help="also write one line per query: query length kmers unique loci genomes_hit best_genome best_frac")
    lo.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    lo.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    plc = sub.add_parser("place", help="which indexed genome an unassembled read set resembles along an anchor genome, bin by bin: the reads "
                                       "joined and counted against the anchor's k-mers and that column joined with the anchor's bitmap rows on "
                                       "the GPU: tab-separated, with a header, chrom start end valid held best best_jaccard second second_jaccard")
    plc.add_argument("index_dir")
    plc.add_argument("anchor", metavar="GENOME", help="the anchor genome (an assembly of the index with bitmap.1)")
    plc.add_argument("reads", metavar="reads.fq", nargs="+", help="FASTQ, four lines per record, plain or .gz")
    plc.add_argument("--chroms", default="", metavar="X,Y", help="the anchor's chromosomes to walk (default: all of them)")
    plc.add_argument("--bin-size", type=int, default=100000, metavar="N", help="positions per bin (default 100000)")
    plc.add_argument("--min-count", type=int, default=2, metavar="C", help="the sample holds a k-mer its reads hold at least C times (default 2)")
    plc.add_argument("--genomes", default="", metavar="A,B", help="the genomes that take part (default: all of them)")
    plc.add_argument("--matrix", metavar="FILE", default=None, help="also write the bins x genomes table of Jaccard indices")
    plc.add_argument("--summary", metavar="FILE", default=None, help="also write one line per genome: genome col both jaccard cont_g cont_s bins_best")
    plc.add_argument("--batch-bytes", type=int, default=None, metavar="N", help="FASTQ text bytes joined at a time (default 2^28)")
    plc.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    plc.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    scn = sub.add_parser("screen", help="which indexed genomes a sample from outside the index holds, and how much of each: the reads (or "
                                        "an assembly) streamed through the table of all genomes' k-mers and counted per k-mer on the GPU: "
                                        "tab-separated, with a header, genome distinct seen containment identity private private_seen "
                                        "private_containment rank")
    scn.add_argument("index_dir")
    scn.add_argument("samples", metavar="sample.fq|sample.fa", nargs="+", help="the sample's files: FASTQ (four lines per record) or FASTA, plain or .gz")
    scn.add_argument("--min-count", type=int, default=None, metavar="C",
                     help="the sample holds a k-mer it holds at least C times, 1 to 255 (default: 2 when a file is FASTQ, else 1)")
    scn.add_argument("--genomes", default="", metavar="A,B", help="the genomes to print (default: all of them; ranks are among all)")
    scn.add_argument("--occupancy", metavar="FILE", default=None, help="also write n, kmers, seen: the k-mers held by exactly n genomes")
    scn.add_argument("--summary", metavar="FILE", default=None, help="also write one comment line per statistic: reads, windows, hits, novel_frac, ...")
    scn.add_argument("--batch-bytes", type=int, default=None, metavar="N", help="FASTQ text bytes joined at a time (default 2^28)")
    scn.add_argument("-o", "--output", metavar="FILE", default=None, help="default: stdout")
    scn.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    nvl = sub.add_parser("novel", help="what a sample from outside the index holds that no indexed genome does: the distinct k-mers of the "
                                       "reads (or an assembly) that miss the table of all genomes' k-mers, counted on the GPU; prints "
                                       "name<TAB>value per statistic: novel_kmers, solid_kmers, solid_windows, error_windows, ...")
    nvl.add_argument("index_dir")
    nvl.add_argument("samples", metavar="sample.fq|sample.fa", nargs="+", help="the sample's files: FASTQ (four lines per record) or FASTA, plain or .gz")
    nvl.add_argument("--min-count", type=int, default=None, metavar="C",
                     help="a k-mer is solid when the sample holds it at least C times: the only error filter (default: 2 when a file is FASTQ, else 1)")
    nvl.add_argument("--spectrum", metavar="FILE", default=None, help="also write depth, kmers: the novel k-mers at every depth 1 to 63 (63: and beyond)")
    nvl.add_argument("--kmers", metavar="FILE", default=None, help="also write kmer, depth: the solid novel k-mers, sorted")
    nvl.add_argument("--regions", metavar="FILE", default=None,
                     help="also write file contig start end kmers bases left_held right_held: the runs of novel k-mers along an assembly (no FASTQ)")
    nvl.add_argument("--min-bases", type=int, default=0, metavar="B", help="regions of at least B bases that lie in novel k-mers only (default 0)")
    nvl.add_argument("--unitigs", metavar="FILE", default=None,
                     help="also write FASTA: the solid novel k-mers compacted on the GPU into unitigs, the non-branching paths of their de Bruijn "
                          "graph (>u1 bases= kmers= depth= circular=), longest first; prints unitigs, unitig_bases, unitig_n50, ... behind the statistics")
    nvl.add_argument("--min-unitig-bases", type=int, default=None, metavar="B", help="unitigs of at least B bases (default 0; needs --unitigs)")
    nvl.add_argument("--clean", action="store_true",
                     help="clip error tips and pop bubbles on the GPU before the compaction (needs --unitigs): a dead-end branch, or the weaker "
                          "of two parallel branches, is dropped when a sibling is deeper by 1 / R or more; prints clipped_tips, clipped_kmers, "
                          "popped_bubbles, popped_kmers, clean_rounds behind the unitig statistics")
    nvl.add_argument("--tip-kmers", type=int, default=None, metavar="T", help="tips of at most T k-mers (1 to 1024; default 2 k; needs --clean)")
    nvl.add_argument("--bubble-kmers", type=int, default=None, metavar="B", help="bubble branches of at most B k-mers (1 to 1024; default 2 k; needs --clean)")
    nvl.add_argument("--clean-ratio", type=float, default=None, metavar="R", help="above 0 and below 1 (default 0.25; needs --clean)")
    nvl.add_argument("--clean-rounds", type=int, default=None, metavar="N", help="rounds at the most, 0 to 64 (default 4; needs --clean)")
    nvl.add_argument("--summary", metavar="FILE", default=None, help="also write the statistics to FILE")
    nvl.add_argument("--batch-bytes", type=int, default=None, metavar="N", help="FASTQ text bytes joined at a time (default 2^28)")
    nvl.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    ad = sub.add_parser("add", help="append the samples of a samples table to an existing index without re-anchoring it: the anchors "
                                    "already there get their rows widened on the GPU by the new samples' columns, new anchors are anchored")
    ad.add_argument("index_dir")
    ad.add_argument("new_samples", metavar="new_samples.tsv", help="name, fasta, optional gff and anchor columns: the NEW samples only")
    ad.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    sb = sub.add_parser("subset", help="write an index of chosen samples of an existing index into a new directory: the kept anchors get "
                                       "their rows narrowed on the GPU, no sequence is read")
    sb.add_argument("index_dir")
    sb.add_argument("-o", "--out", required=True, metavar="out_dir", help="the new index directory (absent or empty)")
    sb.add_argument("--keep", default=None, metavar="A,B,...", help="the samples to keep, in this order")
    sb.add_argument("--drop", default=None, metavar="C,D,...", help="the samples to leave out; the rest keep the index's order")
    sb.add_argument("--anchors", default=None, metavar="A,B", help="write only these of the kept anchors")
    sb.add_argument("--no-sequence-files", action="store_true",
                    help="leave out kmc/bitvec*, genome_dist.tsv, kmer_shared.tsv and kmer_occupancy.tsv instead of refreshing them from the "
                         "kept samples' FASTA files")
    sb.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    um = sub.add_parser("umaps", help="write chrom_umaps.csv and genome_umap.csv of an existing index: nearest neighbours of "
                                      "the bins on the GPU, layout and clusters on the host")
    um.add_argument("index_dir")
    um.add_argument("genomes", nargs="*", help="default: every anchor genome")
    um.add_argument("--device", type=int, default=int(os.environ.get("LOCAL_RANK", "0")))
    it = sub.add_parser("intros", help="call introgressions from k-mer similarity binned on the GPU: `intros call [flags]` "
                                       "(call_introgressions.py's flags) or `intros <config.yaml> [--sweep]`", add_help=False)
    it.add_argument("args", nargs=argparse.REMAINDER)
    ra = sub.add_parser("run_anchor", help="argv-compatible with the reference's cpp/run_anchor")
    ra.add_argument("args", nargs="+")
    ra.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.cmd == "index":
        from .index import KMC, Index
        idx = Index(a.input, prefix=a.prefix, k=a.k, cores=a.cores, prepare=a.prepare,
                    anchor_genomes=a.anchor_genomes, device=a.device, export_kmc=a.export_kmc,
                    kmc=KMC(use_existing=a.use_existing), genome_dist=a.genome_dist, annotate=a.annotate, umaps=a.umaps,
                    kmer_stats=a.kmer_stats)
        idx.run()
        return 0
    if a.cmd == "add":
        if not os.path.isdir(a.index_dir):
            ap.error(f"add: {a.index_dir!r} is not an index directory")
        if not os.path.isfile(a.new_samples):
            ap.error(f"add: no samples table {a.new_samples!r}")
        from .index import Index
        try:
            idx = Index(a.index_dir, mode="w", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"add: {e}")
        try:
            try:
                lines = idx.add(a.new_samples)
            except ValueError as e:
                ap.error(str(e))
        finally:
            idx.close()
        for line in lines:
            print(line)
        return 0
    if a.cmd == "subset":
        if not os.path.isdir(a.index_dir):
            ap.error(f"subset: {a.index_dir!r} is not an index directory")
        from .index import Index
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"subset: {e}")
        try:
            try:
                lines = idx.subset(a.out, keep=a.keep, drop=a.drop, anchors=a.anchors, sequence_files=not a.no_sequence_files)
            except ValueError as e:
                ap.error(str(e))
        finally:
            idx.close()
        for line in lines:
            print(line)
        return 0
    if a.cmd == "dist":
        from .index import Index
        idx = Index(a.index_dir, mode="r", device=a.device)
        try:
            print("Wrote", idx.write_genome_dist(exact=True) if a.exact else idx.write_genome_dist())
        finally:
            idx.close()
        return 0
    if a.cmd == "pangenome":
        if not os.path.isdir(a.index_dir):
            ap.error(f"pangenome: {a.index_dir!r} is not an index directory")
        from . import pangenome
        from .index import Index
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"pangenome: {e}")
        try:
            import pandas as pd
            for n in idx.genome_names:  # (the table is built from the samples' sequences)
                fa = idx[n].fasta
                if pd.isna(fa) or not os.path.isfile(str(fa)):
                    ap.error(f"pangenome: sample {n!r} of {a.index_dir} has no sequence file to count k-mers of ({fa})")
            stats = idx._kmer_stats_raw()
            shared, genomes = pangenome.frames(stats, idx.genome_names)
        finally:
            idx.close()
        if a.matrix:
            shared.to_csv(a.matrix, sep="\t", index_label="name")
        if a.occupancy:
            pangenome.occupancy_frame(stats).to_csv(a.occupancy, sep="\t", index=False)
        genomes.to_csv(sys.stdout, sep="\t", index_label="name")
        return 0
    if a.cmd == "annotate":
        from .index import Index
        idx = Index(a.index_dir, mode="r", device=a.device)
        try:
            idx[a.genome].run_annotate(a.gff_file, nogene=a.nogene)
        finally:
            idx.close()
        return 0
    if a.cmd == "umaps":
        from .index import Index
        idx = Index(a.index_dir, mode="r", device=a.device)
        try:
            names = a.genomes or [n for n in idx.genome_names if idx[n].anchored]
            for n in names:
                if n not in idx.genomes or not idx[n].anchored:
                    ap.error(f"umaps: {n!r} is not an anchor genome of {a.index_dir}")
            for n in names:
                print("Wrote", *idx[n].write_umaps())
        finally:
            idx.close()
        return 0
    if a.cmd == "find":
        if a.whole == (a.chrom is not None):
            ap.error("find: give a chromosome or --whole (and no region with --whole)")
        if a.density is not None and (a.start is not None or a.min_len != 1 or a.max_gap != 0):
            ap.error("find: --density takes whole chromosomes and no --min-len / --max-gap")
        from .index import Index
        have, lack = ([g for g in v.split(",") if g] for v in (a.have, a.lack))
        idx = Index(a.index_dir, mode="r", device=a.device)
        try:
            if a.genome not in idx.genomes or not idx[a.genome].anchored:
                ap.error(f"find: {a.genome!r} is not an anchor genome of {a.index_dir}")
            for g in have + lack:
                if g not in idx.genome_names:
                    ap.error(f"find: unknown genome {g!r} (the index has {', '.join(idx.genome_names)})")
            try:
                if a.density is not None:
                    out = idx.pattern_density(a.genome, have, lack, a.min_have, a.max_lack, None if a.chrom is None else [a.chrom],
                                              a.step, a.density)
                else:
                    out = idx.find_pattern(a.genome, have, lack, a.min_have, a.max_lack, a.chrom, a.start, a.end, a.step,
                                           a.min_len, a.max_gap)
            except (ValueError, KeyError) as e:
                ap.error(f"find: {e}")
        finally:
            idx.close()
        out.to_csv(a.output if a.output else sys.stdout, sep="\t", header=False, index=False)
        return 0
    if a.cmd == "gaps":
        if a.whole == (a.chrom is not None):
            ap.error("gaps: give a chromosome or --whole (and no region with --whole)")
        from .index import Index
        chosen = [g for g in a.genomes.split(",") if g]
        idx = Index(a.index_dir, mode="r", device=a.device)
        try:
            if a.genome not in idx.genomes or not idx[a.genome].anchored:
                ap.error(f"gaps: {a.genome!r} is not an anchor genome of {a.index_dir}")
            for g in chosen:
                if g not in idx.genome_names:
                    ap.error(f"gaps: unknown genome {g!r} (the index has {', '.join(idx.genome_names)})")
            k = int(idx.k)
            try:
                out, spectrum, summary = idx[a.genome].absence_tables(chosen or None, a.chrom, a.start, a.end, 1,
                                                                      k - 1 if a.min_len is None else a.min_len, a.max_len,
                                                                      4 * k if a.maxlen is None else a.maxlen)
            except (ValueError, KeyError) as e:
                ap.error(f"gaps: {e}")
            if a.summary and summary is None:
                ap.error(f"gaps: --summary needs a spectrum that reaches past k: --maxlen above {k}")
        finally:
            idx.close()
        if a.spectrum:
            spectrum.to_csv(a.spectrum, sep="\t", index=False)
        if a.summary:
            summary.to_csv(a.summary, sep="\t", index=False)
        out.to_csv(a.output if a.output else sys.stdout, sep="\t", header=False, index=False)
        return 0
    if a.cmd == "search":
        if not os.path.isdir(a.index_dir):
            ap.error(f"search: {a.index_dir!r} is not an index directory")
        if not os.path.isfile(a.queries):
            ap.error(f"search: no query file {a.queries!r}")
        if not 0.0 <= a.min_frac <= 1.0:
            ap.error("search: --min-frac is a fraction, 0 to 1")
        if a.batch_bases is not None and a.batch_bases < 1:
            ap.error("search: --batch-bases must be at least 1")
        from .index import Index
        chosen = [g for g in a.genomes.split(",") if g]
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"search: {e}")
        try:
            import pandas as pd
            for g in chosen:
                if g not in idx.genome_names:
                    ap.error(f"search: unknown genome {g!r} (the index has {', '.join(idx.genome_names)})")
            for n in idx.genome_names:  # (the table is built from the samples' sequences)
                fa = idx[n].fasta
                if pd.isna(fa) or not os.path.isfile(str(fa)):
                    ap.error(f"search: sample {n!r} of {a.index_dir} has no sequence file to take k-mers of ({fa})")
            try:
                out, matrix, summary = idx.search(a.queries, chosen or None, a.min_frac, a.by, a.batch_bases)
            except (ValueError, KeyError) as e:
                ap.error(f"search: {e}")
        finally:
            idx.close()
        if a.matrix:
            matrix.to_csv(a.matrix, sep="\t", index_label="query")
        if a.summary:
            summary.to_csv(a.summary, sep="\t", index=False)
        out.to_csv(a.output if a.output else sys.stdout, sep="\t", index=False)
        return 0
    if a.cmd == "copies":
        if (a.targets is None) == (a.genes is None):
            ap.error("copies: give exactly one of targets.fa and --genes GENOME")
        if not os.path.isdir(a.index_dir):
            ap.error(f"copies: {a.index_dir!r} is not an index directory")
        if a.targets is not None and not os.path.isfile(a.targets):
            ap.error(f"copies: no target file {a.targets!r}")
        if a.k is not None and not 1 <= a.k <= 32:
            ap.error(f"copies: k={a.k} (1 to 32)")
        from .index import Index
        from . import copies
        chosen = [g for g in a.genomes.split(",") if g]
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"copies: {e}")
        try:
            if a.genes is not None and a.genes not in idx.genomes:
                ap.error(f"copies: unknown genome {a.genes!r} (the index has {', '.join(idx.genome_names)})")
            try:
                if a.genes is not None:
                    got = idx[a.genes].gene_copies(chosen or None, a.k, bool(a.track))
                else:
                    got = idx.copies(a.targets, chosen or None, a.k, bool(a.track))
            except (ValueError, KeyError) as e:
                ap.error(f"copies: {e}")
        finally:
            idx.close()
        out, matrix, summary = got[:3]
        if a.matrix:
            copies.matrix_text(matrix).to_csv(a.matrix, sep="\t", index_label="target")
        if a.summary:
            summary.to_csv(a.summary, sep="\t", index=False)
        if a.track:
            ng = max(1, len(matrix.columns))
            with open(a.track, "w") as f:
                f.write(copies.TRACK_HEADER + "\n")
                f.writelines(line + "\n" for line in copies.track_lines(list(matrix.index), out["length"].to_numpy()[::ng], idx.k if a.k is None else a.k,
                                                                        list(matrix.columns), got[3]))
        copies.long_text(out).to_csv(a.output if a.output else sys.stdout, sep="\t", index=False)
        return 0
    if a.cmd == "place":
        if not os.path.isdir(a.index_dir):
            ap.error(f"place: {a.index_dir!r} is not an index directory")
        for r in a.reads:
            if not os.path.isfile(r):
                ap.error(f"place: no read file {r!r}")
        if a.bin_size < 1 or a.min_count < 1 or (a.batch_bytes is not None and a.batch_bytes < 1):
            ap.error("place: --bin-size, --min-count and --batch-bytes must be positive")
        from .index import Index
        from . import place
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"place: {e}")
        try:
            try:
                main_, matrix, summary, stats = idx.place(a.anchor, a.reads, [c for c in a.chroms.split(",") if c] or None, a.bin_size,
                                                          a.min_count, [g for g in a.genomes.split(",") if g] or None, a.batch_bytes)
            except (ValueError, KeyError) as e:
                ap.error(f"place: {e}")
        finally:
            idx.close()
        if a.matrix:
            place.write_matrix(matrix, a.matrix)
        if a.summary:
            place.write_summary(summary, stats, a.summary)
        place.write_main(main_, a.output if a.output else sys.stdout)
        return 0
    if a.cmd == "screen":
        if not os.path.isdir(a.index_dir):
            ap.error(f"screen: {a.index_dir!r} is not an index directory")
        for r in a.samples:
            if not os.path.isfile(r):
                ap.error(f"screen: no sample file {r!r}")
        if (a.min_count is not None and not 1 <= a.min_count <= 255) or (a.batch_bytes is not None and a.batch_bytes < 1):
            ap.error("screen: --min-count is 1 to 255, --batch-bytes positive")
        from .index import Index
        from . import screen
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"screen: {e}")
        try:
            import pandas as pd
            for n in idx.genome_names:  # (the table is built from the samples' sequences)
                fa = idx[n].fasta
                if pd.isna(fa) or not os.path.isfile(str(fa)):
                    ap.error(f"screen: sample {n!r} of {a.index_dir} has no sequence file to take k-mers of ({fa})")
            try:
                main_, occupancy, stats = idx.screen(a.samples, a.min_count, [g for g in a.genomes.split(",") if g] or None, a.batch_bytes)
            except (ValueError, KeyError) as e:
                ap.error(f"screen: {e}")
        finally:
            idx.close()
        if a.occupancy:
            screen.write_occupancy(occupancy, a.occupancy)
        if a.summary:
            screen.write_summary(stats, a.summary)
        screen.write_main(main_, a.output if a.output else sys.stdout)
        return 0
    if a.cmd == "novel":
        if not os.path.isdir(a.index_dir):
            ap.error(f"novel: {a.index_dir!r} is not an index directory")
        for r in a.samples:
            if not os.path.isfile(r):
                ap.error(f"novel: no sample file {r!r}")
        if (a.min_count is not None and not 1 <= a.min_count <= 0xFFFFFFFF) or (a.batch_bytes is not None and a.batch_bytes < 1) or a.min_bases < 0:
            ap.error("novel: --min-count is 1 to 2^32 - 1, --batch-bytes positive, --min-bases not negative")
        if a.min_unitig_bases is not None and not a.unitigs:
            ap.error("novel: --min-unitig-bases needs --unitigs FILE")
        if a.min_unitig_bases is not None and a.min_unitig_bases < 0:
            ap.error("novel: --min-unitig-bases not negative")
        clean_flags = {"--tip-kmers": a.tip_kmers, "--bubble-kmers": a.bubble_kmers, "--clean-ratio": a.clean_ratio, "--clean-rounds": a.clean_rounds}
        if a.clean and not a.unitigs:
            ap.error("novel: --clean needs --unitigs FILE")
        for flag, v in clean_flags.items():
            if v is not None and not a.clean:
                ap.error(f"novel: {flag} needs --clean")
        if a.clean_ratio is not None and not 0.0 < a.clean_ratio < 1.0:
            ap.error("novel: --clean-ratio is above 0 and below 1")
        if any(v is not None and not 1 <= v <= 1024 for v in (a.tip_kmers, a.bubble_kmers)) or (a.clean_rounds is not None and not 0 <= a.clean_rounds <= 64):
            ap.error("novel: --tip-kmers and --bubble-kmers are 1 to 1024, --clean-rounds 0 to 64")
        from .index import Index, is_fastq
        from . import novel
        if a.regions and any(is_fastq(r) for r in a.samples):
            ap.error("novel: --regions needs an assembly: " + ", ".join(repr(r) for r in a.samples if is_fastq(r)) + " is FASTQ")
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"novel: {e}")
        try:
            import pandas as pd
            for n in idx.genome_names:  # (the table is built from the samples' sequences)
                fa = idx[n].fasta
                if pd.isna(fa) or not os.path.isfile(str(fa)):
                    ap.error(f"novel: sample {n!r} of {a.index_dir} has no sequence file to take k-mers of ({fa})")
            try:
                stats, spectrum, kmers, regions, *unitigs = idx.novel(a.samples, a.min_count, a.batch_bytes, kmers=bool(a.kmers),
                                                                      regions=bool(a.regions), min_bases=a.min_bases, unitigs=bool(a.unitigs),
                                                                      min_unitig_bases=a.min_unitig_bases or 0,
                                                                      clean={"tip_kmers": a.tip_kmers, "bubble_kmers": a.bubble_kmers,
                                                                             "ratio": a.clean_ratio, "rounds": a.clean_rounds} if a.clean else None)
            except ValueError as e:
                ap.error(f"novel: {e}")
        finally:
            idx.close()
        if a.spectrum:
            novel.write_spectrum(spectrum, a.spectrum)
        if a.kmers:
            novel.write_kmers(kmers, a.kmers)
        if a.regions:
            novel.write_regions(regions, a.regions)
        if a.summary:
            novel.write_summary(stats, a.summary)
        novel.write_stats(stats, sys.stdout)
        if a.unitigs:
            novel.write_unitigs(unitigs[0], a.unitigs)
            sys.stdout.writelines(line + "\n" for line in novel.unitig_stat_lines(novel.unitig_stats(unitigs[0])))
            if a.clean:
                sys.stdout.writelines(line + "\n" for line in novel.clean_stat_lines(unitigs[1]))
        return 0
    if a.cmd == "locate":
        if (a.queries is None) == (a.genes is None):
            ap.error("locate: give exactly one of queries.fa and --genes GENOME")
        if not os.path.isdir(a.index_dir):
            ap.error(f"locate: {a.index_dir!r} is not an index directory")
        if a.queries is not None and not os.path.isfile(a.queries):
            ap.error(f"locate: no query file {a.queries!r}")
        if a.k is not None and not 1 <= a.k <= 32:
            ap.error(f"locate: k={a.k} (1 to 32)")
        if a.min_kmers < 1:
            ap.error("locate: --min-kmers must be at least 1")
        if not 0.0 <= a.min_frac <= 1.0:
            ap.error("locate: --min-frac is a fraction, 0 to 1")
        from .index import Index
        from . import locate
        chosen = [g for g in a.genomes.split(",") if g]
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"locate: {e}")
        try:
            if a.genes is not None and a.genes not in idx.genomes:
                ap.error(f"locate: unknown genome {a.genes!r} (the index has {', '.join(idx.genome_names)})")
            params = (a.k, a.min_run, a.max_gap, a.max_shift, a.min_kmers, a.min_frac)
            try:
                if a.genes is not None:
                    loci, matrix, summary = idx[a.genes].gene_loci(chosen or None, *params)
                else:
                    loci, matrix, summary = idx.locate(a.queries, chosen or None, *params)
            except (ValueError, KeyError) as e:
                ap.error(f"locate: {e}")
        finally:
            idx.close()
        if a.matrix:
            matrix.to_csv(a.matrix, sep="\t", index_label="query")
        if a.summary:
            summary.to_csv(a.summary, sep="\t", index=False)
        if a.paf:
            text = "".join(line + "\n" for line in locate.paf_lines(loci, loci.attrs["chrom_lens"]))
            if a.output:
                with open(a.output, "w") as f:
                    f.write(text)
            else:
                sys.stdout.write(text)
        else:
            loci.to_csv(a.output if a.output else sys.stdout, sep="\t", index=False)
        return 0
    if a.cmd == "synteny":
        if a.min_len < 1:
            ap.error("synteny: --min-len must be at least 1")
        if a.blocks and a.variants:
            ap.error("synteny: --blocks and --variants exclude each other")
        if a.vcf and not a.variants:
            ap.error("synteny: --vcf needs --variants")
        if not a.blocks and (a.paf or (not a.variants and (a.min_run is not None or a.max_gap is not None or a.max_shift is not None))):
            ap.error("synteny: --paf, --min-run, --max-gap and --max-shift need --blocks (the last three: or --variants)")
        if a.variants and a.min_len != 1:
            ap.error("synteny: --min-len goes with runs or blocks, not with --variants")
        from .index import Index
        idx = Index(a.index_dir, mode="r", device=a.device)
        try:
            for g in (a.genome_a, a.genome_b):
                if g not in idx.genomes:
                    ap.error(f"synteny: unknown genome {g!r} (the index has {', '.join(idx.genome_names)})")
            chroms = [[c for c in s.split(",") if c] or None for s in (a.chroms_a, a.chroms_b)]
            try:
                if a.variants:
                    out, summary, totals, lens = idx.synteny_variants_tables(
                        a.genome_a, a.genome_b, chroms[0], chroms[1], a.k, 1 if a.min_run is None else a.min_run,
                        1000 if a.max_gap is None else a.max_gap, 100 if a.max_shift is None else a.max_shift)
                elif a.blocks:
                    out, summary, totals, lens = idx.synteny_blocks_tables(
                        a.genome_a, a.genome_b, chroms[0], chroms[1], a.k, 1 if a.min_run is None else a.min_run,
                        1000 if a.max_gap is None else a.max_gap, 100 if a.max_shift is None else a.max_shift, a.min_len)
                else:
                    out, summary, totals = idx.synteny_tables(a.genome_a, a.genome_b, chroms[0], chroms[1], a.k, a.min_len)
            except (ValueError, KeyError) as e:
                ap.error(f"synteny: {e}")
        finally:
            idx.close()
        from . import synteny
        if a.summary:
            synteny.write_summary(a.summary, summary, totals)
        if a.paf or a.vcf:
            f = open(a.output, "w") if a.output else sys.stdout
            try:
                f.writelines(line + "\n" for line in (synteny.paf_lines(out, *lens) if a.paf else synteny.vcf_lines(out, lens[0], a.genome_b)))
            finally:
                if a.output:
                    f.close()
            return 0
        if a.variants:
            out = out.replace({"ref": {"": "-"}, "alt": {"": "-"}})  # (an empty allele: no empty field in the table)
        out.to_csv(a.output if a.output else sys.stdout, sep="\t", header=False, index=False)
        return 0
    if a.cmd == "genotype":
        if not os.path.isdir(a.index_dir):
            ap.error(f"genotype: {a.index_dir!r} is not an index directory")
        if a.genome_a == a.genome_b:
            ap.error(f"genotype: {a.genome_a!r} against itself has no variants")
        for r in a.samples:
            if not os.path.isfile(r):
                ap.error(f"genotype: no sample file {r!r}")
        if not 0.0 < a.min_frac <= 1.0:
            ap.error("genotype: --min-frac is above 0 and at most 1")
        if a.min_count is not None and a.min_count < 1:
            ap.error("genotype: --min-count must be at least 1")
        if a.k is not None and not 1 <= a.k <= 32:
            ap.error("genotype: -k is 1 to 32")
        if a.sample is not None and not a.vcf:
            ap.error("genotype: --sample needs --vcf")
        if a.batch_bytes is not None and a.batch_bytes < 1:
            ap.error("genotype: --batch-bytes must be positive")
        from .index import Index, is_fastq
        from . import genotype
        try:
            idx = Index(a.index_dir, mode="r", device=a.device)
        except (ValueError, OSError) as e:
            ap.error(f"genotype: {e}")
        try:
            import pandas as pd
            for g in (a.genome_a, a.genome_b):
                if g not in idx.genomes:
                    ap.error(f"genotype: unknown genome {g!r} (the index has {', '.join(idx.genome_names)})")
                fa = idx[g].fasta
                if pd.isna(fa) or is_fastq(str(fa)) or not os.path.isfile(str(fa)):
                    ap.error(f"genotype: genome {g!r} of {a.index_dir} has no assembly FASTA ({fa})")
            chroms = [[c for c in s.split(",") if c] or None for s in (a.chroms_a, a.chroms_b)]
            try:
                table, summary, stats = idx.genotype(a.genome_a, a.genome_b, a.samples, chroms[0], chroms[1], a.k, a.min_run, a.max_gap,
                                                     a.max_shift, a.min_count, a.min_frac, a.batch_bytes)
                lens_a = dict(zip(idx.seqset_for(a.genome_a).names, (int(n) for n in idx.seqset_for(a.genome_a).lens)))
            except (ValueError, KeyError) as e:
                ap.error(f"genotype: {e}")
        finally:
            idx.close()
        if a.summary:
            genotype.write_summary(summary, stats, a.summary)
        if a.vcf:
            if chroms[0] is not None:
                lens_a = {n: v for n, v in lens_a.items() if n in chroms[0]}
            name = a.sample if a.sample is not None else os.path.basename(a.samples[0])
            f = open(a.output, "w") if a.output else sys.stdout
            try:
                f.writelines(line + "\n" for line in genotype.vcf_lines(table, lens_a, name))
            finally:
                if a.output:
                    f.close()
            return 0
        genotype.write_main(table, a.output if a.output else sys.stdout)
        return 0
    if a.cmd == "patterns":
        if a.whole == (a.chrom is not None):
            ap.error("patterns: give a chromosome or --whole (and no region with --whole)")
        if a.occupancy and (a.top is not None or a.min_rows != 1):
            ap.error("patterns: --occupancy takes no --top / --min-rows")
        if (a.top is not None and a.top < 0) or a.min_rows < 0:
            ap.error("patterns: --top and --min-rows must not be negative")
        from . import patterns
        from .index import Index
        chosen = [g for g in a.genomes.split(",") if g]
        idx = Index(a.index_dir, mode="r", device=a.device)
        try:
            if a.genome not in idx.genomes or not idx[a.genome].anchored:
                ap.error(f"patterns: {a.genome!r} is not an anchor genome of {a.index_dir}")
            for g in chosen:
                if g not in idx.genome_names:
                    ap.error(f"patterns: unknown genome {g!r} (the index has {', '.join(idx.genome_names)})")
            if not chosen and len(idx.genome_names) > patterns.MAX_SELECTED:
                ap.error(f"patterns: the index has {len(idx.genome_names)} genomes and a pattern takes at most "
                         f"{patterns.MAX_SELECTED}: name them with --genomes")
            try:
                keys, counts, selected = idx.pattern_counts(a.genome, chosen or None, a.chrom, a.start, a.end, a.step)
            except (ValueError, KeyError) as e:
                ap.error(f"patterns: {e}")
        finally:
            idx.close()
        if a.occupancy:
            import pandas as pd
            rows = patterns.occupancy(keys, counts, len(selected))
            out = pd.DataFrame({"n": range(len(rows)), "rows": rows})
        else:
            out = patterns.spectrum_frame(keys, counts, selected, a.top, a.min_rows)
            out["genomes"] = [",".join(g for g, b in zip(selected, p) if b == "1") or "-" for p in out["pattern"]]
        out.to_csv(a.output if a.output else sys.stdout, sep="\t", index=False)
        return 0
    if a.cmd == "tree":
        if a.whole == (a.chrom is not None):
            ap.error("tree: give a chromosome or --whole (and no region with --whole)")
        from .index import Index
        idx = Index(a.index_dir, mode="r", device=a.device)
        try:
            tree = idx.region_tree(a.genome, a.chrom, a.start, a.end, a.step)
        finally:
            idx.close()
        if a.matrix:
            tree.counts.to_csv(a.matrix, sep="\t", index_label="name")
        print(tree.newick)
        return 0
    from .index import run_anchor_cli
    return run_anchor_cli(a.args, a.device)


if __name__ == "__main__":
    sys.exit(main())
