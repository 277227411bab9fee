// offline.hip — libdeepmod_hip.so, training and the offline commands: the BiLSTM trainer, the cluster trainer, getfeatures (the .xy writer), the
// line splitter of every text parsed on the device (textlines.hip.inc) and the tiled writer of every text formatted per position
// (textout.hip.inc on textout.inc), predict (the .xy parser), the resident gather of train --resident,
// siteperf, merge, bsperf, bslabels (their line grammars and routines: siteperf.inc, bedmerge.inc, bsperf.inc, bslabels.inc on bedline.inc), motifs (motifs.inc), diffmod (diffmod.inc, and diffrep.inc for --replicates).  Interface to the other
// units: host.h.
#include "train.hip.inc"
#include "cluster_train.hip.inc"
#include "xyrows.inc"
#include "xyrows.hip.inc"
#include "textlines.hip.inc"
#include "textout.hip.inc"
#include "xyparse.hip.inc"
#include "xygather.hip.inc"
#include "siteperf.hip.inc"
#include "bedmerge.hip.inc"
#include "bsperf.hip.inc"
#include "bslabels.hip.inc"
#include "motifs.hip.inc"
#include "motifs.inc"
#include "diffmod.hip.inc"
#include "diffmod.inc"
#include "diffrep.hip.inc"
#include "diffrep.inc"
