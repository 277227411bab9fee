#!/usr/bin/env python
"""DeepMod (MI355X-native hot path) command line.

Keeps the `detect` sub-command of the reference's bin/DeepMod.py (flag names and defaults of
bin/DeepMod.py:304-338) for the path this build implements: per-read BiLSTM modification calling on
the GPU and the per-position BED summary.  `--wrkBase` holds feature containers (*.dmfeat.npz, see
deepmod_amd/predstore.py) because FAST5 reading and alignment are out of scope here.

`train` (flags of bin/DeepMod.py:341-350 plus --seed and --batchsize) trains the BiLSTM on the GPU from the
reference's *.xy.gz feature files and writes TF-bundle checkpoints `detect --modfile` loads
(deepmod_amd/train.py).  Beside every checkpoint lies <prefix>.train.json, the schedule's position: --resume
CKPT_PREFIX continues a stopped run from it, checkpoint for checkpoint the bytes of the uninterrupted run;
--startFrom CKPT_PREFIX runs the whole schedule from an existing model's weights; --validate K (with --test)
keeps K held-out windows on the GPU, scores them at every checkpoint (<prefix>.valid.json) and names the
best one.  --resident 1 loads the training files once through the GPU parser and keeps them on the GPU: a step
sends window ids, not windows, and the checkpoints are the default run's byte for byte.

`getfeatures` (flags and defaults of bin/DeepMod.py:354-375) writes those *.xy.gz / *.xy.ind files from raw
containers (*.dmraw.npz, event tables or --move), a reference and known modified positions - a motif
(--motifORPos 1) or position lists (--motifORPos 2): signal statistics, row selection and text on one GPU,
alignment walk and gzip on --threads host threads (deepmod_amd/getfeatures.py).  Only --fnum 7 and
--SignalGroup simple; --region takes a contig name; an --outFolder that already holds */*.xy.gz is refused
(the reference deletes it).

`predict` scores a checkpoint on labelled *.xy.gz files (the reference's unwired pred_entry / mPred): text parsing, row
selection and the classifier on one GPU, gunzip on --threads host threads; --test takes the value `train` was given and
evaluates what `train` left out.  Writes <outFolder>/<FileID>_mpred.txt (the reference's tp / fp / fn / tn lines) and
<FileID>_mpred.json (deepmod_amd/predict.py).

`traincluster --predFile <prefix> --motifFolder <dir> --truth <bedMethyl[,..]> [--chr chr1[,..]] [--heldout chrN[,..]] [--cov 5]
[--keep_prob 0.7] [--epochs 1] [--batchsize 4096] [--seed 0]` fits the CpG-cluster model of `detect --clusterCpG` /
hm_cluster_predict.py on the sites that have bisulfite truth: the training graph the reference ships, on one GPU; row order,
epochs, dropout stream and initial draw are this project's own, fixed by --seed (deepmod_amd/cluster_train.py).

`siteperf --predFolder RUN --control C1[,C2..] --Ref genome.fa --motif Cg --ModinMotif 0 [--chr NAME] [--start S --end E] [--cov 1,5]
--outFolder O --FileID id` is DeepMod_tools/cal_EcoliDetPerf.py: per-site ROC AUC and average precision of a modified run against control
runs, for every site category and for motif sites only, at each coverage threshold.  The BED lines are parsed, classified and counted on one
GPU into integer histograms; the numbers are exact functions of those (deepmod_amd/siteperf.py).  Writes <O>/<id>_siteperf.txt (the
reference's lines) and <O>/<id>_siteperf.json (the curves); no plots.

`merge --predFolder RUNS --Base C --FileID SUM [--chr chr1,chr2,..] [--Ref genome.fa --clusterCpG [CKPT_PREFIX]] [--threads T]` is
DeepMod_tools/sum_chr_mod.py for a data set that was split over several detect runs: per contig the *.<chr>+.<Base>.bed / *.<chr>-.<Base>.bed files one to
three levels below RUNS are parsed, summed and written as RUNS/SUM.<chr>.<Base>.bed on one GPU, byte for byte the tool's file; with --clusterCpG the
summed counters also go through the CpG-cluster stage (RUNS/SUM_clusterCpG.<chr>.C.bed, the output of generate_motif_pos.py and
hm_cluster_predict.py on the merged file).  RUNS/SUM_merge.json lists files, lines and kernel times (deepmod_amd/merge.py).

`bsperf --predFolder RUNS --truth rep1.bed,rep2.bed[,..] --Base C --outFolder O --FileID id [--chr chr1,chr2,..] [--cov 1,5,10] [--predCov 1]
[--methylated 90] [--unmethylated 0] [--Ref genome.fa] [--clusterCpG [CKPT_PREFIX]] [--threads T]` is Step 5 of Example 3 of the reference's
docs/Reproducibility.md, for which it ships no script: the predicted percentages of the runs below RUNS (summed as `merge` sums them) against 1 to 4
whole-genome bisulfite bedMethyl replicates.  A site is completely methylated if its percentage is >= --methylated in every replicate,
completely un-methylated if it is <= --unmethylated in every replicate, at a bisulfite coverage >= each --cov threshold in every replicate.  The
truth text is parsed, joined with the counters and counted on one GPU; O/id_bsperf.txt has ROC AUC, average precision, Pearson r and RMSE per
threshold, raw and (with --clusterCpG) after the CpG-cluster stage on the same sites; O/id_bsperf.json has every counter and curve
(deepmod_amd/bsperf.py).  Hand in the mod_pos.* files of `detect` runs: the files `merge` and sum_chr_mod.py write drop every position whose
modified count is 0, which are exactly the unmethylated sites.

`bslabels --truth rep1.bed,rep2.bed[,..] --Ref genome.fa --Base C --outFolder O --FileID id [--chr chr1,chr2,..] [--motif CG --ModinMotif 0] [--cov 5]
[--methylated 90] [--unmethylated 0]` writes the three position lists `getfeatures --motifORPos 2 --fulmod F --anymod A --nomod N` reads, from 1 to 4
whole-genome bisulfite bedMethyl replicates read by `bsperf`'s rules: per contig O/id.fulmod.<chr>.txt (sites of the motif at >= --methylated in every
replicate, every replicate at coverage >= --cov), O/id.nomod.<chr>.txt (<= --unmethylated in every replicate, at that coverage) and O/id.anymod.<chr>.txt
(every other site of the motif that has a record in a replicate: getfeatures --posneg 1 labels a position of anymod not at all, so every site one
cannot be sure of belongs there).  Lines are `chr strand pos` with the 0-based position, classified and formatted on one GPU; O/id_bslabels.json has the
line and class counters (deepmod_amd/bslabels.py).  The workflow closes: bslabels -> getfeatures -> train -> detect -> bsperf.

`motifs --predFolder RUNS [--control C1[,C2..]] --Ref genome.fa --Base A --outFolder O --FileID id [--chr ..] [--flank 3,3] [--cov 5] [--minPct 50]
[--maxCtrlPct 10] [--minFrac 50] [--minSites 20] [--maxMotifs 8] [--threads T]` answers the question every command above leaves to the user: in which
sequence contexts are the modified bases?  The *.<chr>+.<Base>.bed / *.<chr>-.<Base>.bed files below RUNS are summed as `merge` sums them, the control
folders pooled the same way; one sweep per contig on one GPU counts, per oriented context of --flank bases around every --Base, the sites tested
(coverage >= --cov in the sample and in the controls) and those called modified (percentage >= --minPct, and <= --maxCtrlPct in the controls).  The motifs
are then picked from the counts by an exact integer rule (deepmod_amd/motifs.py).  O/id_motifs.txt lists them with the ready
`--motif <label> --ModinMotif <k>` arguments of siteperf / getfeatures; O/id_motifs.json has every counter, the non-zero contexts and notes.  Hand in the
mod_pos.* files of `detect` runs (summed files drop every position with a modified count of 0).  The threshold defaults have not been tuned on real data.

`diffmod --predFolder RUNS --control C1[,C2..] --Base C --outFolder O --FileID id [--chr ..] [--Ref genome.fa] [--cov 5] [--fdr 0.05] [--minDelta 10]
[--all 0|1] [--threads T]` answers what a user with a sample and a control asks first: which sites differ, and how sure are we?  The files below RUNS
are summed as `merge` sums them, the control folders pooled into a second pair of tables; every (strand, position) with --cov reads in both gets the
two-sided p of Fisher's exact test on one GPU (R's fisher.test rule) and a Benjamini-Hochberg q-value over all tested keys.  O/id_diffmod.txt lists the
keys with q <= --fdr whose percentages differ by --minDelta points or more (--all 1: every tested key); O/id_diffmod.json has the counters, the p
histogram and notes (deepmod_amd/diffmod.py).  Hand in mod_pos.* files.  Pooling runs before an exact test ignores the variation between
replicates: the p-values are those of the pooled counts.

`diffmod --replicates 1 --predFolder S1,S2[,..] --control C1,C2[,..] [--minReps a,b] ...` keeps the replicates apart instead: every folder of
--predFolder is one sample replicate and every folder of --control one control replicate (1 to 8 each, 3 or more together).  A replicate counts at a
key when it has --cov reads there; a key with a sample and b control replicates that count (--minReps, default all of them) gets the quasi-binomial
F test of a two-group logistic model on one GPU: the deviance of the pooled 2 x 2 table over the dispersion phi = max(1, Pearson X2 / (replicates
- 2)) between the replicates, p from F(1, replicates - 2).  The report gains the columns repA, repB and phi; q-values, --fdr, --minDelta and --all
work as before.  The test reads 16 bytes of device memory per position and replicate
(the tables of an open contig hold 24).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def non_negative(value, name):
    if value < 0:
        raise SystemExit('Error: --%s must be non-negative (got %d)' % (name, value))


def build_parser():
    parser = argparse.ArgumentParser(prog='DeepMod.py', description='Detect DNA modifications from nanopore reads '
                                     '(per-read BiLSTM calling + per-position summary) on AMD MI355X.')
    sub = parser.add_subparsers(dest='cmd')
    com = argparse.ArgumentParser(add_help=False)
    com.add_argument('--outLevel', type=int, choices=[0, 1, 2, 3], default=2, help='0 debug, 1 info, 2 warning, 3 error')
    com.add_argument('--wrkBase', help='working base folder with the input files')
    com.add_argument('--FileID', default='mod', help='unique id of this run')
    com.add_argument('--outFolder', default='./mod_output', help='default output folder')
    com.add_argument('--recursive', type=int, choices=[0, 1], default=1, help='search sub-folders (up to 3 levels)')
    com.add_argument('--threads', type=int, default=4, help='number of worker processes')
    com.add_argument('--files_per_thread', type=int, default=1000, help='input files per worker batch')
    com.add_argument('--windowsize', type=int, default=21, help='window size (odd)')
    com.add_argument('--alignStr', choices=['bwa', 'minimap2'], default='minimap2', help='aligner run on raw containers when on PATH; otherwise side-car <container>.sam files are read')
    com.add_argument('--SignalGroup', choices=['simple', 'rundif'], default='simple', help='accepted for compatibility')
    com.add_argument('--move', action='store_true', default=False,
                     help='raw containers: take the events from the basecaller move tables (Guppy and later: Move, first_sample_template and the Fastq sequence) instead of an event table')
    det = sub.add_parser('detect', parents=[com], help='detect modifications')
    det.add_argument('--Ref', help='reference genome FASTA (raw containers: reference bases of the aligned reads)')
    det.add_argument('--predDet', type=int, choices=[0, 1], default=1, help='1: predict + summarise; 0: summarise only')
    det.add_argument('--predpath', default=None, help='prediction folder for --predDet 0')
    det.add_argument('--modfile', default=None, help='checkpoint prefix of the trained model (TF bundle)')
    det.add_argument('--fnum', type=int, default=7, help='features per event')
    det.add_argument('--hidden', type=int, default=100, help='LSTM hidden units')
    det.add_argument('--basecall_1d', default='Basecall_1D_000', help='accepted for compatibility')
    det.add_argument('--basecall_2strand', default='BaseCalled_template', help='accepted for compatibility')
    det.add_argument('--region', default=None, help='regions of interest, e.g. chr1:1:100000;chr2:10000')
    det.add_argument('--ConUnk', default=True, help='also process contigs whose names contain _ - / :')
    det.add_argument('--outputlayer', default='', choices=['', 'sigmoid'], help="only '' is built")
    det.add_argument('--Base', default='C', choices=['A', 'C', 'G', 'T'], help='base of interest')
    det.add_argument('--mod_cluster', default=0, type=int, choices=[0, 1], help='only 0 is built')
    det.add_argument('--gpus', type=int, default=None, help='GPUs to spread the workers over (default: all visible)')
    det.add_argument('--storePred', type=int, choices=[0, 1], default=0,
                     help='0 (default): streaming detect - per-position counters stay on the GPUs, one RCCL reduce per contig x strand, '
                          'no per-read files; 1: also keep the per-read prediction tables and index files of the reference '
                          '(needed for a later --predDet 0 run)')
    det.add_argument('--clusterCpG', nargs='?', const='', default=None, metavar='CKPT_PREFIX',
                     help='--Base C with --Ref: after the mod_pos.* files, also write <outFolder>/<FileID>_clusterCpG.<chr>.C.bed per contig - the output of '
                          'sum_chr_mod.py, generate_motif_pos.py (motif CG) and hm_cluster_predict.py on this run, computed from the counters on the GPU. '
                          'CKPT_PREFIX: checkpoint prefix of the cluster model (default: DEEPMOD_CLUSTER_MODEL)')
    det.set_defaults(func=mDetect)
    trn = sub.add_parser('train', parents=[com], help='train a modification classifier on the GPU',
                         description='Train the BiLSTM on *.xy.gz feature files (the format getfeatures of the reference writes): forward, backpropagation through '
                                     'time and Adam as HIP kernels, fp32.  --wrkBase "a,b;c": groups separated by ;, folders of a group by , (the larger group leads). '
                                     'The AUC of the progress line is the exact ROC statistic of the displayed batch, not the 200-threshold approximation of '
                                     'tf.metrics.auc.  Initial values are TF1\'s distributions drawn from numpy (--seed): TensorFlow\'s own stream cannot be reproduced.')
    trn.add_argument('--wrkBase2', help='accepted for compatibility (the reference parses and never reads it): name further groups in --wrkBase "a;b"')
    trn.add_argument('--fnum', type=int, default=7, help='features per event')
    trn.add_argument('--hidden', type=int, default=100, help='LSTM hidden units')
    trn.add_argument('--modfile', default=None, help='accepted and ignored with a note: the reference never restores it')
    trn.add_argument('--test', default=None, help="independent testing: 'E,a,b' leaves positions a..b (Mb) out, 'P,pct' uses pct %% of the files")
    trn.add_argument('--outputlayer', default='', choices=['', 'sigmoid'], help="only '' is built")
    trn.add_argument('--unbalanced', type=int, default=0, choices=[1, 0], help='1: class weights [0.1, 0.9] inside the loss')
    trn.add_argument('--seed', type=int, default=0, help='seed of the initial values (numpy generator)')
    trn.add_argument('--batchsize', type=int, default=2048, help='windows per training step (the reference fixes 2048): the leading group is cut into steps of batchsize .. 2 batchsize - 1 windows, a step of another group can be larger by a file; the device tape (158,400 B per window) is sized for 2 batchsize - 1 and grows to the largest step met')
    trn.add_argument('--resume', default=None, metavar='CKPT_PREFIX',
                     help='continue the run that wrote this checkpoint (its .train.json and bundle: weights, Adam slots, step count, reader positions) with the same '
                          '--wrkBase, --test, --batchsize and --unbalanced: every later checkpoint is byte for byte the uninterrupted run\'s; --seed is not used')
    trn.add_argument('--startFrom', default=None, metavar='CKPT_PREFIX',
                     help='start the whole schedule from the 14 variables of this TF bundle (a published model, or a checkpoint of this command) instead of a fresh '
                          'initialisation; Adam starts from zero; --seed is not used; excludes --resume')
    trn.add_argument('--validate', type=int, default=0, metavar='K',
                     help='with --test: keep at least K windows of the held-out data on the GPU (whole files, one per folder in turn) and score them at every checkpoint '
                          'as predict would: <prefix>.valid.json, and <outFolder>/<FileID>_valid.json with the best checkpoint by AUC (default 0: off)')
    trn.add_argument('--resident', type=int, default=0, choices=[0, 1],
                     help='1: load every training file once, before the first step, through the GPU parser (as predict loads its files; gunzip on --threads host '
                          'threads) and keep it on the GPU at 28 B per row + 5 B per window; every step then gathers its windows there from 8 B of window id '
                          'each.  Checkpoints and .train.json are byte for byte those of the default (0: files are read on the host, round by round, in every '
                          'epoch).  A labelled row without a whole window is reported while loading.  DEEPMOD_RESIDENT_BYTES=N ends the run before its first '
                          'step when the files need more than N bytes')
    trn.set_defaults(func=mTrain)
    prd = sub.add_parser('predict', parents=[com], help='score a trained model on labelled *.xy.gz feature files',
                         description='Evaluate a checkpoint on labelled *.xy.gz files: per file the text is parsed, the labelled rows are selected and their '
                                     'windows classified on one GPU (precision: DEEPMOD_PRECISION, as detect).  --wrkBase: folders separated by , or ; - files in '
                                     'sorted order, no shuffle.  Writes <outFolder>/<FileID>_mpred.txt (tp= fp= fn= tn= per piece of at most 2048 windows) and '
                                     '<FileID>_mpred.json (counts, accuracy, precision, recall, exact ROC AUC).')
    prd.add_argument('--fnum', type=int, default=7, help='features per event')
    prd.add_argument('--hidden', type=int, default=100, help='LSTM hidden units')
    prd.add_argument('--modfile', default=None, help='checkpoint prefix of the trained model (TF bundle)')
    prd.add_argument('--test', default=None, help="the value train was given: 'E,a,b' evaluates only positions a..b (Mb), 'P,pct' the files train did not use")
    prd.add_argument('--outputlayer', default='', choices=['', 'sigmoid'], help="only '' is built")
    prd.set_defaults(func=mPredict)
    gf = sub.add_parser('getfeatures', parents=[com], help='get labelled features of all raw reads for training',
                        description='Write the *.xy.gz / *.xy.ind training files from raw containers (*.dmraw.npz), a reference and known modified positions: '
                                    'per worker batch of --files_per_thread inputs a folder <outFolder>/<batch id>/.  One GPU; --threads host threads load, walk '
                                    'alignments and gzip.  Inputs are taken in sorted order.  An --outFolder that already holds */*.xy.gz is refused (the reference '
                                    'deletes the folder).')
    gf.add_argument('--posneg', type=int, default=0, choices=[0, 1], help='the positive (1) or negative (0) class')
    gf.add_argument('--size_per_batch', type=int, default=1, help='size (unit: 10^7 bytes at 80 bytes per row) of a feature file')
    gf.add_argument('--fnum', type=int, default=7, help='features per event (only 7 is built)')
    gf.add_argument('--region', type=str, help='contig of interest (the start:end part of the reference cannot work under Python 3 and is refused)')
    gf.add_argument('--basecall_1d', default='Basecall_1D_000', help='accepted for compatibility')
    gf.add_argument('--basecall_2strand', default='BaseCalled_template', help='accepted for compatibility')
    gf.add_argument('--motifORPos', type=int, default=1, help='motif (1) or position lists (2) for the modified bases')
    gf.add_argument('--motif', default='CG', type=str, help='the motif of interest')
    gf.add_argument('--ModinMotif', default=0, type=int, help='position of the modified base in the motif')
    gf.add_argument('--Ref', help='reference genome FASTA')
    gf.add_argument('--fulmod', type=str, help='file pattern of completely modified positions (lines: chr strand pos)')
    gf.add_argument('--anymod', type=str, help='file pattern of partially modified positions')
    gf.add_argument('--nomod', type=str, help='file pattern of unmodified positions')
    gf.set_defaults(func=mGetFeatures)
    tcl = sub.add_parser('traincluster', parents=[com], help='fit the CpG-cluster model (detect --clusterCpG, hm_cluster_predict.py) on the GPU',
                         description='Fit the second-stage MLP 14 -> 100 -> 20 -> 1 on the sites of a DeepMod BED that have bisulfite truth: the training graph the '
                                     'reference ships (dropout, mean squared error, Adam) on one GPU.  The order of the rows, the number of epochs, the dropout random '
                                     'stream and the draw of the initial values are this project\'s own, all fixed by --seed (the reference ships no training '
                                     'script and TensorFlow\'s random stream cannot be reproduced).  Writes <outFolder>/Cg.cov<cov>.nb25-<epoch> (TF bundles with the '
                                     'Adam slots, loadable by detect --clusterCpG and hm_cluster_predict.py) after every epoch and <outFolder>/<FileID>_cluster_train.json.')
    tcl.add_argument('--predFile', default=None, help='prefix of the DeepMod BED files, as the first argument of hm_cluster_predict.py: <prefix>.<chr>.C.bed')
    tcl.add_argument('--motifFolder', default=None, help='folder with motif_<chr>_C.bed (generate_motif_pos.py)')
    tcl.add_argument('--truth', default=None, help='bisulfite bedMethyl file(s), separated by commas (11 columns; the first line is skipped)')
    tcl.add_argument('--chr', default='chr1', help='contigs to train on, separated by commas (default chr1, as the shipped model)')
    tcl.add_argument('--heldout', default='', help='contigs scored after every epoch at keep_prob 1 (MSE, Pearson r), never trained on')
    tcl.add_argument('--cov', type=int, default=5, help='least coverage of a truth row (hm_cluster_predict.py:18)')
    tcl.add_argument('--keep_prob', type=float, default=0.7, help='dropout keep probability in (0, 1] (the shipped model: 0.7)')
    tcl.add_argument('--epochs', type=int, default=1, help='passes over the rows (the project\'s own choice; default 1)')
    tcl.add_argument('--batchsize', type=int, default=4096, help='rows per step (hm_cluster_predict.py:16)')
    tcl.add_argument('--seed', type=int, default=0, help='seeds the initial values, the order of the rows and the dropout masks: the same seed gives the same bytes')
    tcl.set_defaults(func=mTrainCluster)
    spf = sub.add_parser('siteperf', parents=[com], help='site-level ROC / PR of a run against control runs (cal_EcoliDetPerf.py) on the GPU',
                         description='Per-site ROC AUC and average precision of the methylation percentage of a modified run against control runs, as '
                                     'DeepMod_tools/cal_EcoliDetPerf.py prints them: for all seven site categories and for motif sites only, at every coverage '
                                     'threshold.  Writes <outFolder>/<FileID>_siteperf.txt (the reference\'s lines; the PNG names are labels, nothing is drawn) and '
                                     '<outFolder>/<FileID>_siteperf.json (counts, curves, histograms).')
    spf.add_argument('--predFolder', default=None, help='folder of the modified run: mod_pos.*.<B>.bed in it, one or two levels below')
    spf.add_argument('--control', default=None, help='folder(s) of the control runs, separated by commas; their coverage is summed per site')
    spf.add_argument('--Ref', help='reference genome FASTA')
    spf.add_argument('--motif', default='Cg', help='motif, as the reference types it (default Cg)')
    spf.add_argument('--ModinMotif', type=int, default=0, help='offset of the modified base in the motif; the base there names the files and must be upper case')
    spf.add_argument('--chr', default=None, help='evaluate this contig only (default: every contig of the FASTA)')
    spf.add_argument('--start', type=int, default=None, help='first position of the region (inclusive; needs --chr)')
    spf.add_argument('--end', type=int, default=None, help='last position of the region (inclusive; needs --chr)')
    spf.add_argument('--cov', default='1,5', help='coverage thresholds, ascending, at most 8 (default 1,5)')
    spf.set_defaults(func=mSitePerf)
    mrg = sub.add_parser('merge', parents=[com], help='sum the BED files of several detect runs per contig (sum_chr_mod.py) on the GPU',
                         description='Per contig: every *.<chr>-.<Base>.bed and *.<chr>+.<Base>.bed one to three levels below --predFolder is parsed on one GPU, '
                                     'coverage and modified count are summed per (position, strand), and <predFolder>/<FileID>.<chr>.<Base>.bed is written as '
                                     'DeepMod_tools/sum_chr_mod.py writes it (positions with a modified count of 0 dropped; an empty file for a contig without '
                                     'input).  Writes <predFolder>/<FileID>_merge.json (files, lines, notes, kernel times).  --threads host threads read ahead.')
    mrg.add_argument('--predFolder', default=None, help='folder of the runs: the BED files are searched one to three levels below it')
    mrg.add_argument('--Base', default='C', choices=['A', 'C', 'G', 'T'], help='base of interest: names the files')
    mrg.add_argument('--chr', default=None, help='contigs to merge, separated by commas (default chr1..22, chrX, chrY, chrM)')
    mrg.add_argument('--Ref', default=None, help='reference genome FASTA: a line beyond its contig is refused (without it the tables grow with the files)')
    mrg.add_argument('--clusterCpG', nargs='?', const='', default=None, metavar='CKPT_PREFIX',
                     help='--Base C with --Ref: also write <predFolder>/<FileID>_clusterCpG.<chr>.C.bed per contig with a site - the output of generate_motif_pos.py '
                          '(motif CG) and hm_cluster_predict.py on the merged file, computed from the summed counters on the GPU.  CKPT_PREFIX: checkpoint '
                          'prefix of the cluster model (default: DEEPMOD_CLUSTER_MODEL)')
    mrg.set_defaults(func=mMerge)
    bsp = sub.add_parser('bsperf', parents=[com], help='score a run against whole-genome bisulfite replicates (Reproducibility.md, Example 3, Step 5) on the GPU',
                         description='Per contig: every *.<chr>-.<Base>.bed and *.<chr>+.<Base>.bed one to three levels below --predFolder is summed as merge sums '
                                     'them, joined with the bedMethyl replicates of --truth and counted on one GPU.  Hand in the mod_pos.* files of detect runs: '
                                     'the files merge and sum_chr_mod.py write drop every position whose modified count is 0, and that removes exactly the '
                                     'unmethylated sites.  Writes <outFolder>/<FileID>_bsperf.txt (per threshold: sites scored and without a prediction, ROC AUC, '
                                     'average precision, Pearson r, RMSE) and <outFolder>/<FileID>_bsperf.json (inputs, lines, every counter, the curves, kernel times).')
    bsp.add_argument('--predFolder', default=None, help='folder of the runs: the BED files are searched one to three levels below it')
    bsp.add_argument('--truth', default=None, help='1 to 4 whole-genome bisulfite bedMethyl replicates, separated by commas (11 columns; the first line is skipped)')
    bsp.add_argument('--Base', default='C', choices=['A', 'C', 'G', 'T'], help='base of interest: names the files')
    bsp.add_argument('--chr', default=None, help='contigs to score, separated by commas, at most 64 (default chr1..22, chrX, chrY, chrM)')
    bsp.add_argument('--cov', default='1,5,10', help='thresholds on the bisulfite coverage of every replicate, ascending, at most 8 (default 1,5,10)')
    bsp.add_argument('--predCov', type=int, default=1, help='least summed coverage of a predicted site (default 1)')
    bsp.add_argument('--methylated', type=int, default=90, help='a site is completely methylated at this percentage or more in every replicate (default 90)')
    bsp.add_argument('--unmethylated', type=int, default=0, help='a site is completely un-methylated at this percentage or less in every replicate (default 0)')
    bsp.add_argument('--Ref', default=None, help='reference genome FASTA: fixes the contig lengths (without it a contig is as long as the largest position seen + 1)')
    bsp.add_argument('--clusterCpG', nargs='?', const='', default=None, metavar='CKPT_PREFIX',
                     help='--Base C with --Ref: also score the percentages of the CpG-cluster stage on the same sites, side by side with the raw ones.  '
                          'CKPT_PREFIX: checkpoint prefix of the cluster model (default: DEEPMOD_CLUSTER_MODEL)')
    bsp.set_defaults(func=mBsPerf)
    bsl = sub.add_parser('bslabels', parents=[com], help='training position lists (getfeatures --fulmod / --anymod / --nomod) from bisulfite replicates on the GPU',
                         description='Per contig: the bedMethyl replicates of --truth, read by the rules of bsperf, are joined per (strand, position) with the sites '
                                     'of the motif in --Ref and classified on one GPU.  Writes <outFolder>/<FileID>.fulmod.<chr>.txt, .anymod.<chr>.txt and '
                                     '.nomod.<chr>.txt (lines `chr strand pos`, 0-based, as getfeatures --motifORPos 2 reads them) and '
                                     '<outFolder>/<FileID>_bslabels.json (inputs, line and class counters, notes, kernel times).')
    bsl.add_argument('--truth', default=None, help='1 to 4 whole-genome bisulfite bedMethyl replicates, separated by commas (11 columns; the first line is skipped)')
    bsl.add_argument('--Ref', default=None, help='reference genome FASTA (needed: getfeatures refuses a position that is not in the reference)')
    bsl.add_argument('--Base', default='C', choices=['A', 'C', 'G', 'T'], help='base of interest')
    bsl.add_argument('--chr', default=None, help='contigs to write lists for, separated by commas, at most 64 (default: those of chr1..22, chrX, chrY, chrM in --Ref)')
    bsl.add_argument('--motif', default=None, help='motif a site lies in, 1 to 8 letters of A, C, G, T (default: --Base alone)')
    bsl.add_argument('--ModinMotif', type=int, default=0, help='offset of the modified base in the motif; the letter there is --Base (default 0)')
    bsl.add_argument('--cov', type=int, default=5, help='least bisulfite coverage in every replicate of a fulmod / nomod site, 1 to 65535 (default 5)')
    bsl.add_argument('--methylated', type=int, default=90, help='fulmod: this percentage or more in every replicate (default 90)')
    bsl.add_argument('--unmethylated', type=int, default=0, help='nomod: this percentage or less in every replicate (default 0)')
    bsl.set_defaults(func=mBsLabels)
    mot = sub.add_parser('motifs', parents=[com], help='de novo discovery of the modified motifs from a run and its controls on the GPU',
                         description='Per contig: every *.<chr>-.<Base>.bed and *.<chr>+.<Base>.bed one to three levels below --predFolder (and below every '
                                     '--control folder, pooled) is summed as merge sums them and joined with --Ref on one GPU: per oriented sequence context of '
                                     '--flank bases around each --Base, the sites tested and the sites called modified.  The motifs are picked from those counts by '
                                     'an integer rule: the pattern with the fewest fixed letters among those with --minSites modified sites that are --minFrac '
                                     'percent of its tested sites, its contexts removed, and again.  Writes <outFolder>/<FileID>_motifs.txt (rank, motif, '
                                     'ModinMotif, label, sites, modified, percent, the arguments for siteperf / getfeatures) and <outFolder>/<FileID>_motifs.json.  '
                                     'Hand in the mod_pos.* files of detect runs.  The threshold defaults have not been tuned on real data.')
    mot.add_argument('--predFolder', default=None, help='folder of the sample\'s runs: the BED files are searched one to three levels below it')
    mot.add_argument('--control', default=None, help='folder(s) of control runs, separated by commas; pooled (default: none)')
    mot.add_argument('--Ref', default=None, help='reference genome FASTA (needed: the contexts are read from it)')
    mot.add_argument('--Base', default='A', choices=['A', 'C', 'G', 'T'], help='the modified base: names the files (default A)')
    mot.add_argument('--chr', default=None, help='contigs, separated by commas (default: every contig of --Ref)')
    mot.add_argument('--flank', default='3,3', help='bases upstream,downstream of the modified base in a context, 8 in all at most (default 3,3)')
    mot.add_argument('--cov', type=int, default=5, help='least coverage of a tested site, in the sample and in the pooled controls (default 5)')
    mot.add_argument('--minPct', type=int, default=50, help='a site is called modified at this percentage or more in the sample (default 50)')
    mot.add_argument('--maxCtrlPct', type=int, default=10, help='and at this percentage or less in the controls (default 10)')
    mot.add_argument('--minFrac', type=int, default=50, help='a motif: at least this percentage of its tested sites is modified (default 50)')
    mot.add_argument('--minSites', type=int, default=20, help='a motif: at least this many modified sites (default 20)')
    mot.add_argument('--maxMotifs', type=int, default=8, help='motifs reported at most (default 8)')
    mot.set_defaults(func=mMotifs)
    dif = sub.add_parser('diffmod', parents=[com], help='per-site differential modification of a run against controls: Fisher\'s exact test on the GPU, BH q-values',
                         description='Per contig: every *.<chr>-.<Base>.bed and *.<chr>+.<Base>.bed one to three levels below --predFolder is summed as merge sums '
                                     'them, every --control folder pooled the same way into a second pair of tables.  Every (strand, position) with --cov reads in '
                                     'both gets the two-sided p of Fisher\'s exact test (the rule of R\'s fisher.test) on one GPU, and a Benjamini-Hochberg q-value '
                                     'over all tested keys of the run.  Writes <outFolder>/<FileID>_diffmod.txt (chr, 0-based pos, strand, coverage, modified and '
                                     'percentage of the sample and of the controls, delta, p, q of every key with q <= --fdr whose percentages differ by --minDelta '
                                     'points or more) and <outFolder>/<FileID>_diffmod.json (counters, the p histogram, notes, kernel times).  Hand in the mod_pos.* '
                                     'files of detect runs (summed files drop every position with a modified count of 0).  Pooling runs before an exact test ignores '
                                     'the variation between replicates: the p-values are those of the pooled counts.  --replicates 1 keeps the replicates apart: '
                                     'every folder of --predFolder and of --control is one replicate (1 to 8 each, 3 or more together), and every key with '
                                     '--minReps replicates of --cov reads gets a quasi-binomial F test (the deviance of the pooled table over the dispersion between '
                                     'the replicates); the report gains the columns repA, repB and phi.  No motif restriction, and the two strands of a CpG are not '
                                     'merged.')
    dif.add_argument('--predFolder', default=None, help='folder of the sample\'s runs: the BED files are searched one to three levels below it (--replicates 1: one folder per sample '
                                                         'replicate, separated by commas)')
    dif.add_argument('--control', default=None, help='folder(s) of control runs, separated by commas; pooled, or one replicate each under --replicates 1 (needed)')
    dif.add_argument('--Ref', default=None, help='reference genome FASTA: only fixes the contigs and their lengths (default: the tables grow with the files)')
    dif.add_argument('--Base', default='C', choices=['A', 'C', 'G', 'T'], help='the modified base: names the files (default C)')
    dif.add_argument('--chr', default=None, help='contigs, separated by commas (default: those of --Ref, or those the sample\'s file names hold)')
    dif.add_argument('--cov', type=int, default=5, help='least coverage of a tested key, in the sample and in the pooled controls (default 5)')
    dif.add_argument('--fdr', type=float, default=0.05, help='a key is listed at this q-value or less, above 0 and at most 1 (default 0.05)')
    dif.add_argument('--minDelta', type=int, default=10, help='and when its percentages differ by this many points or more (default 10)')
    dif.add_argument('--all', type=int, default=0, help='1: write every tested key with its q, whatever --fdr and --minDelta (default 0)')
    dif.add_argument('--replicates', type=int, default=0, help='1: every folder of --predFolder (separated by commas) and of --control is one replicate, tested by a '
                                                                'quasi-binomial F test; 0: the folders are pooled (default 0)')
    dif.add_argument('--minReps', default=None, help='with --replicates 1: a,b - a key is tested with at least a sample and b control replicates of --cov reads '
                                                     '(default: every replicate)')
    dif.set_defaults(func=mDiffmod)
    return parser


def mDiffmod(args):
    from deepmod_amd import diffmod
    mo = {k: getattr(args, k) for k in ('predFolder', 'Ref', 'Base', 'outFolder', 'FileID', 'cov', 'fdr', 'minDelta', 'all', 'threads', 'replicates', 'minReps')}
    mo['chr'] = [c for c in (args.chr or '').split(',') if c] or None
    mo['control'] = [c for c in (args.control or '').split(',') if c]
    try:
        diffmod.diffmod(mo)                              # checks the options, then refuses without a gfx950 GPU
    except diffmod.DiffmodError as exc:
        raise SystemExit('Error: %s' % exc)


def mMotifs(args):
    from deepmod_amd import motifs
    mo = {k: getattr(args, k) for k in ('predFolder', 'Ref', 'Base', 'outFolder', 'FileID', 'flank', 'cov', 'minPct', 'maxCtrlPct', 'minFrac', 'minSites', 'maxMotifs',
                                         'threads')}
    mo['chr'] = [c for c in (args.chr or '').split(',') if c] or None
    mo['control'] = [c for c in (args.control or '').split(',') if c]
    try:
        motifs.motifs(mo)                                # checks the options (the FASTA is read once), then refuses without a gfx950 GPU
    except motifs.MotifsError as exc:
        raise SystemExit('Error: %s' % exc)


def mBsLabels(args):
    from deepmod_amd import bslabels
    mo = {k: getattr(args, k) for k in ('Ref', 'Base', 'outFolder', 'FileID', 'motif', 'ModinMotif', 'cov', 'methylated', 'unmethylated', 'threads')}
    mo['chr'] = [c for c in (args.chr or '').split(',') if c] or None
    mo['truth'] = [p for p in (args.truth or '').split(',') if p]
    try:
        bslabels.bslabels(mo)                            # checks the options (the FASTA is read once), then refuses without a gfx950 GPU
    except bslabels.BsLabelsError as exc:
        raise SystemExit('Error: %s' % exc)


def mBsPerf(args):
    from deepmod_amd import bsperf
    try:
        cov = tuple(int(v) for v in args.cov.split(',') if v.strip() != '')
    except ValueError:
        raise SystemExit('Error: bsperf: --cov takes integers separated by commas (got %r)' % args.cov)
    mo = {k: getattr(args, k) for k in ('predFolder', 'Base', 'outFolder', 'FileID', 'predCov', 'methylated', 'unmethylated', 'Ref', 'clusterCpG', 'threads')}
    mo['chr'] = [c for c in (args.chr or '').split(',') if c] or None
    mo['truth'] = [p for p in (args.truth or '').split(',') if p]
    mo['cov'] = cov
    if not mo['predFolder']:
        raise SystemExit('Error: bsperf: --predFolder, the folder of the runs, is needed')
    try:
        bsperf.check_options(mo)
        from deepmod_amd import _lib
        if _lib.load().dm_device_count() < 1:
            raise SystemExit('Error: no gfx950 GPU visible (this build has no CPU path)')
        bsperf.bsperf(mo)
    except bsperf.BsPerfError as exc:
        raise SystemExit('Error: %s' % exc)


def mMerge(args):
    from deepmod_amd import merge
    mo = {k: getattr(args, k) for k in ('predFolder', 'Base', 'FileID', 'Ref', 'clusterCpG', 'threads')}
    mo['chr'] = [c for c in (args.chr or '').split(',') if c] or None
    if not mo['predFolder']:
        raise SystemExit('Error: merge: --predFolder, the folder of the runs, is needed')
    try:
        merge.merge_runs(mo)
    except merge.MergeError as exc:
        raise SystemExit('Error: %s' % exc)


def mSitePerf(args):
    from deepmod_amd import siteperf
    try:
        cov = tuple(int(v) for v in args.cov.split(',') if v.strip() != '')
    except ValueError:
        raise SystemExit('Error: siteperf: --cov takes integers separated by commas (got %r)' % args.cov)
    mo = {k: getattr(args, k) for k in ('predFolder', 'Ref', 'motif', 'ModinMotif', 'chr', 'start', 'end', 'outFolder', 'FileID', 'threads')}
    mo['control'] = [c for c in (args.control or '').split(',') if c]
    mo['cov'] = cov
    if not mo['predFolder'] or not mo['control']:
        raise SystemExit('Error: siteperf: --predFolder and --control are needed')
    try:
        siteperf.check_options(mo)
        from deepmod_amd import _lib
        if _lib.load().dm_device_count() < 1:
            raise SystemExit('Error: no gfx950 GPU visible (this build has no CPU path)')
        siteperf.siteperf(mo)
    except siteperf.SitePerfError as exc:
        raise SystemExit('Error: %s' % exc)


def mTrainCluster(args):
    from deepmod_amd import cluster_train
    mo = {k: getattr(args, k) for k in ('outLevel', 'FileID', 'outFolder', 'predFile', 'motifFolder', 'cov', 'keep_prob', 'epochs', 'batchsize', 'seed')}
    for key in ('truth', 'chr', 'heldout'):
        mo[key] = [c for c in (getattr(args, key) or '').split(',') if c]
    cluster_train.train_cluster(mo)


def getfeatures_options(args):
    """moptions of `getfeatures` as bin/DeepMod.py:240-299 of the reference builds them; what this build does not do is refused with one line."""
    if not args.wrkBase or not os.path.isdir(args.wrkBase):
        raise SystemExit('Error: getfeatures: --wrkBase: input folder does not exist')
    mo = {k: getattr(args, k) for k in ('outLevel', 'wrkBase', 'FileID', 'outFolder', 'recursive', 'threads', 'files_per_thread', 'windowsize', 'alignStr',
                                         'SignalGroup', 'move', 'posneg', 'fnum', 'size_per_batch', 'basecall_1d', 'basecall_2strand', 'Ref', 'motifORPos')}
    if mo['fnum'] != 7:
        raise SystemExit('Error: getfeatures: this build supports --fnum 7 only (got %d)' % mo['fnum'])
    if mo['SignalGroup'] != 'simple':
        raise SystemExit('Error: getfeatures: --SignalGroup %s (event re-segmentation) is not built' % mo['SignalGroup'])
    mo['threads'] = max(mo['threads'], 1)
    mo['files_per_thread'] = max(mo['files_per_thread'], 2)          # bin/DeepMod.py:75-78
    if mo['size_per_batch'] < 0.001:
        mo['size_per_batch'] = 0.001                                 # bin/DeepMod.py:252
    if not mo['outFolder'].endswith('/'):
        mo['outFolder'] += '/'
    mo['region'] = [None, None, None]
    if not (args.region is None or args.region.strip() == ''):
        rsp = [v.strip() for v in args.region.split(':')]
        if any(v != '' for v in rsp[1:]):
            raise SystemExit('Error: getfeatures: --region takes a contig name only (got %r): the reference compares the start and end with an int and raises TypeError' % args.region)
        if rsp[0] != '':
            mo['region'][0] = rsp[0]
    if mo['Ref'] is None or not os.path.isfile(mo['Ref']):
        raise SystemExit('Error: getfeatures: --Ref: reference file does not exist (%s)' % mo['Ref'])
    if mo['motifORPos'] == 1:
        mo['motif'] = [args.motif.upper(), args.ModinMotif]
        if not 0 <= args.ModinMotif < len(args.motif):
            raise SystemExit('Error: getfeatures: --ModinMotif %d is no position in the motif %s' % (args.ModinMotif, args.motif))
    elif mo['motifORPos'] == 2:
        missing = [k for k in ('fulmod', 'anymod', 'nomod') if getattr(args, k) is None]
        if missing:
            raise SystemExit('Error: getfeatures: --motifORPos 2 needs --fulmod, --anymod and --nomod (missing: %s)' % ', '.join('--' + k for k in missing))
        mo.update(fulmod=args.fulmod, anymod=args.anymod, nomod=args.nomod)
    else:
        raise SystemExit('Error: getfeatures: --motifORPos %d is not supported (1: motif, 2: position lists)' % mo['motifORPos'])
    from deepmod_amd import getfeatures
    if getfeatures.existing_output(mo['outFolder']):
        raise SystemExit('Error: getfeatures: --outFolder %s already holds */*.xy.gz files (the reference deletes the folder; this build does not)' % mo['outFolder'])
    return mo


def mGetFeatures(args):
    mo = getfeatures_options(args)
    from deepmod_amd import getfeatures
    getfeatures.getFeature_manager(mo)


def train_options(args, cmd='train', keys=('unbalanced', 'modfile', 'seed')):
    """moptions of `train` as bin/DeepMod.py:186-222 of the reference builds them; geometry and output layer are refused as detect refuses them.
    `predict` takes the same folders, geometry and --test (cmd, keys: its own options)."""
    if args is None or not getattr(args, 'wrkBase', None):
        raise SystemExit('Error: %s: --wrkBase: the folders of the *.xy.gz feature files ("a,b;c")' % cmd)
    mo = {k: getattr(args, k) for k in ('outLevel', 'wrkBase', 'FileID', 'outFolder', 'recursive', 'windowsize', 'fnum', 'hidden', 'outputlayer') + tuple(keys)}
    for k in ('windowsize', 'fnum', 'hidden'):
        non_negative(mo[k], k)
    if (mo['fnum'], mo['hidden'], mo['windowsize']) != (7, 100, 21):
        raise SystemExit('Error: this build supports fnum=7 hidden=100 windowsize=21 only (got %s)' % ((mo['fnum'], mo['hidden'], mo['windowsize']),))
    if mo['outputlayer'] in ('sigmoid',):
        raise SystemExit('Error: --outputlayer sigmoid is not used by any shipped model and is not built')
    if cmd == 'train' and args.batchsize < 1:
        raise SystemExit('Error: --batchsize must be positive')
    if not mo['outFolder'].endswith('/'):
        mo['outFolder'] += '/'
    if args.test is not None:                            # bin/DeepMod.py:212-222
        mo['test'] = args.test.split(',')
        if mo['test'][0] == 'E': mo['test'][0] = '-'
        elif mo['test'][0] == 'P': mo['test'][0] = '0'
        else:
            raise SystemExit('Error: Unknown option for test: the first character must be E or P ' + args.test)
        try:
            if mo['test'][0] in ['-']:
                mo['test'][1] = int(mo['test'][1]) * (10 ** 6)
                mo['test'][2] = int(mo['test'][2]) * (10 ** 6)
            else:
                mo['test'][1] = int(mo['test'][1]) / 100.0
        except (IndexError, ValueError):
            raise SystemExit("Error: --test takes 'E,<from Mb>,<to Mb>' or 'P,<percent>' (got %r)" % args.test)
    else:
        mo['test'] = ['N', '100']
    if cmd == 'train':
        mo.update(resume=getattr(args, 'resume', None), startFrom=getattr(args, 'startFrom', None), validate=getattr(args, 'validate', 0),
                  resident=getattr(args, 'resident', 0), threads=max(getattr(args, 'threads', 1) or 1, 1))
        from deepmod_amd import train
        train.check_run_options(mo)
    return mo


def mTrain(args):
    mo = train_options(args)
    from deepmod_amd import _lib, train
    if args.wrkBase2:
        print('Note: --wrkBase2 %s is not read (the reference never reads it either): give further groups as --wrkBase "a;b"' % args.wrkBase2)
    if _lib.load().dm_device_count() < 1:
        raise SystemExit('Error: no gfx950 GPU visible (this build has no CPU path)')
    os.makedirs(mo['outFolder'], exist_ok=True)
    train.mMult_RNN_LSTM_train(mo, batchsize=args.batchsize)


def mPredict(args):
    mo = train_options(args, cmd='predict', keys=('modfile', 'threads'))
    if not mo['modfile'] or not os.path.isfile(mo['modfile'] + '.index'):
        raise SystemExit('Error: predict: --modfile: no TF checkpoint at %r' % mo['modfile'])
    mo['threads'] = max(mo['threads'], 1)
    from deepmod_amd import _lib, predict
    if _lib.load().dm_device_count() < 1:
        raise SystemExit('Error: no gfx950 GPU visible (this build has no CPU path)')
    predict.pred_entry(mo)


def kfd_gpu_count(base='/sys/class/kfd/kfd/topology/nodes'):
    """gfx950 devices this process may open, from /sys/class/kfd (no HIP runtime): topology nodes whose properties are readable (a container's
    device cgroup hides the others) and say gfx_target_version 90500, capped by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES.  None if the
    topology cannot be read."""
    try:
        nodes = os.listdir(base)
    except OSError:
        return None
    n = 0
    for node in nodes:
        try:
            with open(os.path.join(base, node, 'properties')) as fh:
                props = dict(line.split()[:2] for line in fh if len(line.split()) >= 2)
        except OSError:
            continue
        if props.get('gfx_target_version') == '90500' and int(props.get('simd_count', '0')) > 0:
            n += 1
    # A *_VISIBLE_DEVICES filter changes what the runtime shows in ways the topology files do not tell (ROCR and HIP filters compose, an
    # invalid or -1 entry truncates the list): with any of them set the runtime is asked instead
    for var in ('HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES', 'CUDA_VISIBLE_DEVICES', 'GPU_DEVICE_ORDINAL'):
        if os.environ.get(var, '').strip() != '':
            return None
    return n


def mDetect(args):
    from deepmod_amd import _lib, detect
    mo = {k: getattr(args, k) for k in ('outLevel', 'wrkBase', 'FileID', 'outFolder', 'recursive', 'threads', 'files_per_thread',
                                         'windowsize', 'predDet', 'predpath', 'modfile', 'fnum', 'hidden', 'outputlayer', 'Base',
                                         'mod_cluster', 'Ref', 'alignStr', 'SignalGroup', 'basecall_1d', 'basecall_2strand', 'storePred', 'move')}
    for k in ('threads', 'files_per_thread', 'windowsize', 'fnum', 'hidden'):
        non_negative(mo[k], k)
    if mo['threads'] < 1:
        mo['threads'] = 1                                # bin/DeepMod.py:78: at least one worker
    if mo['files_per_thread'] < 2:
        mo['files_per_thread'] = 2                       # bin/DeepMod.py:75-76
    if mo['windowsize'] % 2 == 0:
        raise SystemExit('Error: --windowsize must be odd')
    if not mo['outFolder'].endswith('/'):
        mo['outFolder'] += '/'
    mo['region'] = []                                    # bin/DeepMod.py:153-160: "chr:start:end;chr2:start"
    if args.region is None or len(args.region) == 0:
        mo['region'].append([None, None, None])
    else:
        for mr in args.region.split(';'):
            mr_sp = mr.split(':')
            mo['region'].append([mr_sp[0], int(mr_sp[1]) if len(mr_sp) > 1 else None, int(mr_sp[2]) if len(mr_sp) > 2 else None])
    mo['ConUnk'] = args.ConUnk not in (False, 'False', 'false', '0', 0)
    mo['clusterCpG'] = None
    if args.clusterCpG is not None:
        try:
            mo['clusterCpG'] = detect.cluster_cpg_prefix(args.clusterCpG, mo)
        except ValueError as exc:
            raise SystemExit('Error: --clusterCpG: %s' % exc)
    errs = []
    if mo['predDet'] == 1:
        if not mo['wrkBase'] or not os.path.isdir(mo['wrkBase']):
            errs.append('--wrkBase: input folder does not exist')
        if not mo['modfile'] or not os.path.isfile(mo['modfile'] + '.index'):
            errs.append('--modfile: no TF checkpoint at %r' % mo['modfile'])
    else:
        if not mo['predpath'] or not os.path.isdir(mo['predpath']):
            errs.append('--predpath: prediction folder does not exist')
        else:
            mo['outFolder'] = mo['predpath'].rstrip('/')
    if errs:
        raise SystemExit('Error:\n\t' + '\n\t'.join(errs))
    # how many GPUs: with --gpus N the answer is needed only to refuse N > what is there, and the kernel driver's topology files give it without
    # initialising a HIP runtime in THIS process, which never touches a GPU itself (0.14 s of a 1.8 s run; the rank processes initialise
    # their own).  Without --gpus, or when the files say less than N, the runtime is asked.
    ngpu = kfd_gpu_count() if args.gpus else None
    if ngpu is None or ngpu < args.gpus:
        ngpu = _lib.load().dm_device_count()
    if ngpu < 1:
        raise SystemExit('Error: no gfx950 GPU visible (this build has no CPU path)')
    mo['gpus'] = min(args.gpus, ngpu) if args.gpus else ngpu
    if os.environ.get('DEEPMOD_ONE_DEVICE') == '1' and args.gpus:      # test hook: --gpus N processes, all on device 0 (a one-GPU box; RCCL
        mo['gpus'], mo['one_device'] = args.gpus, True                  # refuses duplicate devices: this exercises start-up, rendezvous and the abort path)
    detect.mDetect_manager(mo)


if __name__ == '__main__':
    parser = build_parser()
    if len(sys.argv) < 2:
        parser.print_help()
        sys.exit(1)
    args = parser.parse_args()
    if not hasattr(args, 'func'):
        parser.print_help()
        sys.exit(1)
    args.func(args)
