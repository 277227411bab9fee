// feed.hip — libdeepmod_hip.so, what feeds `detect`: the signal stage (normalisation, event statistics), the alignment walk and the host row
// builder of a worker batch.  Interface to the other units: host.h.
#include "signal.hip.inc"
#include "readmap.inc"
#include "rowsbatch.inc"
