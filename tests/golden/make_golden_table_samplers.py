#!/usr/bin/env python3
"""Golden tables for tests/test_table_samplers.py: what `sample_grounds`, `sample_payloads`, `sample_actuators`, `sample_delays`,
`sample_noise` and `training_sigma` return for the cases of that file's `tables()`, written from the commit before the samplers
came to share one draw (that commit has no tests/test_table_samplers.py: copy this one into it first).  Regenerate only where a
sampler is meant to change:

    python tests/golden/make_golden_table_samplers.py        # from the repository root; writes table_samplers.npz"""
import os
import sys

import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(here)))

from tests.test_table_samplers import tables  # noqa: E402

np.savez_compressed(os.path.join(here, "table_samplers.npz"), **tables())
