"""`DeepMod.py predict`: score a trained model on labelled *.xy.gz files - the evaluation half of the reference's myMultiBiRNN.py
(pred_entry :465-477, pred_prepare :419-420, mPred :382-414), which the reference never wired to a sub-command.

  pred_entry    the files of --wrkBase, the model, the output path
  pred_prepare  as in the reference: hands mPred its arguments
  mPred         per file: text -> table -> labelled rows -> classes, all on the GPU (xyload.XYLoader: dm_xyload_parse / _select, then
                dm_predict_read_at on the device table under DEEPMOD_PRECISION as detect); tp / fp / fn / tn per piece of at most 2048 windows
                in the reference's lines, and a summary

--test takes the value `train` was given and evaluates what `train` left OUT: E,a,b -> only rows with a Mb < position < b Mb
(getDataFromFile_new's '+'), P,pct -> per folder the files getTFiles1 did not keep under ['0', pct / 100].  --threads host threads read and
gunzip ahead of the device; files are consumed in list order, so the output does not depend on which thread finished first.
"""
from __future__ import annotations

import contextlib
import gzip
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib, train, xyload
from .siteperf import roc_auc

batchsize = 2048                     # myMultiBiRNN.py:12


def predict_files(folder, moptions):
    """The *.xy.gz files of one folder `predict` reads, in getTFiles1's order: all of them, or under ['0', fraction] those getTFiles1
    does not keep for training."""
    with contextlib.redirect_stdout(io.StringIO()):
        found = train.getTFiles1(folder, dict(moptions, test=['N', '100']))
        kept = set(train.getTFiles1(folder, moptions)) if moptions['test'][0] == '0' else set()
    files = [f for f in found if f not in kept] if moptions['test'][0] == '0' else found
    print("%s: %d feature files" % (folder, len(files)))
    sys.stdout.flush()
    return files


def loader_options(moptions):
    """moptions as the loader reads them: the region `train --test E` left out is the region kept here."""
    test = list(moptions['test'])
    if test[0] == '-':
        test[0] = '+'
    return dict(moptions, test=test)


def piece_lines(cls, label, name):
    """mPred's lines of one file (:398-412): np.array_split into int(n / batchsize) + 1 pieces -> (lines, [tp, fp, fn, tn])."""
    lines, total = [], np.zeros(4, np.int64)
    pieces = int(len(cls) / batchsize) + 1
    for c, y in zip(np.array_split(cls, pieces), np.array_split(label, pieces)):
        counts = [int(((c == 1) & (y == 1)).sum()), int(((c == 1) & (y != 1)).sum()), int(((c != 1) & (y == 1)).sum()), int(((c != 1) & (y != 1)).sum())]
        lines.append('tp=%d fp=%d fn=%d tn=%d %s\n' % (*counts, name))
        total += counts
    return lines, total


def finish_stats(stats, total, probs, labels, model):
    """mPred's summary from the counts [tp, fp, fn, tn] and the per-file probabilities and labels, in file order (`train --validate` writes the
    same figures): accuracy, precision, recall, the exact ROC AUC (None unless both labels occur) and the precision the model ran."""
    from . import model as _model
    tp, fp, fn_, tn = (int(v) for v in total)
    stats.update(tp=tp, fp=fp, fn=fn_, tn=tn, accuracy=(tp + tn) / max(stats['windows'], 1), precision=tp / max(tp + fp, 1), recall=tp / max(tp + fn_, 1))
    lab = np.concatenate(labels) if labels else np.zeros(0, np.uint8)
    both = 0 < int(lab.sum()) < len(lab)
    stats['auc'] = float(roc_auc(lab, np.concatenate(probs))) if both else None
    names = {v: k for k, v in _model.BiLSTMModel.PRECISIONS.items()}
    stats['precision_mode'] = names.get(model.get_info(_lib.DM_INFO_PRECISION), 'unknown')
    return stats


def read_text(fn):
    with open(fn, 'rb') as fh:
        return gzip.decompress(fh.read())               # zlib releases the GIL


def mPred(mfbase, mffolder, accuracy, X, Y, test_gzfile2, pf, num_input, auc_op, mpre, mspf, init_l, mfpred, timesteps, moptions):
    from . import model as _model
    sess = _model.new_session(int(moptions.get('device', 0)))
    loader = None
    try:
        new_saver = _model.import_meta_graph(mfbase + '.meta')
        new_saver.restore(sess, mfbase)
        loader = xyload.XYLoader(sess.device)
        lopt = loader_options(moptions)
        files = [fn for group in test_gzfile2 for fn in group]
        threads = max(int(moptions.get('threads', 1)), 1)
        stats = dict(files=len(files), fallback_files=0, rows=0, windows=0)
        total, probs, labels = np.zeros(4, np.int64), [], []
        with open(pf, 'w') as pfwriter, ThreadPoolExecutor(threads) as pool:
            ahead = []                                   # at most 2 * threads texts in flight
            nxt = 0
            for _ in files:
                while nxt < len(files) and len(ahead) < 2 * threads:
                    ahead.append((files[nxt], pool.submit(read_text, files[nxt])))
                    nxt += 1
                fn, fut = ahead.pop(0)
                rows, n, fallback = loader.load(fut.result(), lopt, fn)
                stats['rows'] += rows
                stats['fallback_files'] += int(fallback)
                if n < 1:
                    continue
                prob1, cls, label = loader.classify(sess.model)       # 6 bytes per window; the table stays on the device
                lines, counts = piece_lines(cls, label, fn)
                pfwriter.writelines(lines)
                pfwriter.flush()
                total += counts
                stats['windows'] += n
                probs.append(prob1)
                labels.append(label)
        return finish_stats(stats, total, probs, labels, sess.model)
    finally:
        if loader is not None:
            loader.close()
        sess.close()


def pred_prepare(moptions, test_file, accuracy, X, Y, auc_op, mpre, mspf, init_l, mfpred):
    return mPred(moptions['modfile'][0], moptions['modfile'][1], accuracy, X, Y, test_file, moptions['outFolder'] + moptions['FileID'] + '_mpred.txt',
                 moptions['fnum'], auc_op, mpre, mspf, init_l, mfpred, moptions['windowsize'], moptions)


def pred_entry(moptions):
    from . import model as _model
    tfiles = [[fn for folder in moptions['wrkBase'].replace(';', ',').split(',') if folder for fn in predict_files(folder, moptions)]]
    init, init_l, loss_op, accuracy, train_op, X, Y, saver, auc_op, mpre, mspf, mfpred = \
        _model.mCreateSession(moptions['fnum'], moptions['hidden'], moptions['windowsize'], moptions)
    if not isinstance(moptions['modfile'], list):       # :472-475
        cut = moptions['modfile'].rfind('/')
        moptions['modfile'] = [moptions['modfile'], './' if cut == -1 else moptions['modfile'][:cut + 1]]
    os.makedirs(moptions['outFolder'], exist_ok=True)
    stats = pred_prepare(moptions, tfiles, accuracy, X, Y, auc_op, mpre, mspf, init_l, mfpred)
    with open(moptions['outFolder'] + moptions['FileID'] + '_mpred.json', 'w') as fh:
        json.dump(stats, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(stats, sort_keys=True))
    sys.stdout.flush()
    return stats
