"""The normalisation against implementations this project did not write, on the CPU: the recorded answers of
Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm, Speech2TextFeatureExtractor.utterance_cmvn and SeamlessM4TFeatureExtractor
(tests/golden/features/norm_*.npz, written by tools/make_norm_goldens.py) against the production kernels under the wave simulator
and against the numpy restatement, in both layouts.  Every live cell lies in the interval around the outside value that DESIGN.md
4.15 derives (norm_cases.Outside); every padding cell is the padding value.  The file reads the fixtures only."""
import numpy as np
import pytest

import norm_cases as nc
import simlib_norm as sn


@pytest.mark.parametrize("layout", (sn.CT, sn.TC))
@pytest.mark.parametrize("name", nc.OUTSIDE)
def test_the_simulator_gives_the_recorded_outside_answer(name, layout):
    c = nc.outside(name)
    a = nc.as_layout(c.x32, layout)
    sn.norm_windows(a, c.valid, layout, c.o)
    got = nc.from_layout(a, layout)
    assert nc.same_words(got, sn.restate(c.x32, c.valid, c.o)[0])
    c.check(got, "simulator, layout %d" % layout)


@pytest.mark.parametrize("name", nc.OUTSIDE)
def test_the_float64_reference_gives_the_recorded_outside_answer(name):
    """The outside's own share of the interval alone holds the reference: the two float64 (or exact) evaluations of one formula."""
    c = nc.outside(name)
    ref = sn.reference(c.x, c.valid, c.o)[0]
    n = c.valid[0]
    assert np.all(np.abs(ref - c.want)[..., :n] <= (c.allow - c.ours)[..., :n])


def test_the_wav2vec2_input_is_the_pcm_over_32768():
    c = nc.outside("wav2vec2")
    assert np.array_equal(c.x32[0, 0, :c.valid[0]], c.pcm.astype(np.float32) / np.float32(32768.0)) and np.all(c.x32[0, 0, c.valid[0]:] == 0)
