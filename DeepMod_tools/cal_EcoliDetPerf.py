#!/usr/bin/env python
"""Same command line as the reference's DeepMod_tools/cal_EcoliDetPerf.py:
    python cal_EcoliDetPerf.py <run folder> <genome.fa> <motif> <offset> <contig or ''> <start or -1> <end or -1> <figure folder> <control[,control..]>
Prints the reference's `basetype=` / AUC / ap= lines and writes them to <figure folder>/cal_EcoliDetPerf_siteperf.txt, the curves to
cal_EcoliDetPerf_siteperf.json beside it; the PNG names in the lines are labels, no plot is drawn and neither R nor sklearn is needed.  The work
is `DeepMod.py siteperf` (deepmod_amd/siteperf.py): BED lines parsed, classified and counted on one GPU.  A region needs a contig here."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmod_amd import _lib, siteperf  # noqa: E402

try:
    mo = siteperf.shim_options(sys.argv[1:])
    siteperf.check_options(mo)
    if _lib.load().dm_device_count() < 1:
        sys.exit('Error: no gfx950 GPU visible (this build has no CPU path)')
    siteperf.siteperf(mo)
except siteperf.SitePerfError as exc:
    sys.exit('Error: %s' % exc)
