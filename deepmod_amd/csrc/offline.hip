// offline.hip — libdeepmod_hip.so, training and the offline commands: the BiLSTM trainer, the cluster trainer, getfeatures (the .xy writer), predict
// (the .xy parser), the resident gather of train --resident, siteperf, merge, bsperf.  Interface to the other units: host.h.
#include "train.hip.inc"
#include "cluster_train.hip.inc"
#include "xyrows.inc"
#include "xyrows.hip.inc"
#include "xyparse.hip.inc"
#include "xygather.hip.inc"
#include "siteperf.hip.inc"
#include "bedmerge.hip.inc"
#include "bsperf.hip.inc"
