"""Alias: ``unsupervised_keypoints.visualize`` is ``stablekeypoints_amd.visualize`` (reference ``unsupervised_keypoints/visualize.py``)."""
import sys

from stablekeypoints_amd import visualize as _impl

sys.modules[__name__] = _impl
