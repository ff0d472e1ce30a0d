"""The reflected front ends on the GPU against the recorded outside answers (tests/golden/features/reflected_*.npz;
outside_reflected.py says what is outside-held and what is not): the fixture's PCM as a FLAC stream, opened with open_streams and read
with read_mel from sample 0 with a length past the stream's end, as Kaldi's features of a whole utterance need, in both layouts; every
cell inside outside_cases.py's kernel interval around the outside value, with the vacuity cap as it is."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import outside_cases as oc
import outside_reflected as orf
from test_gpu_outside_features import _btm, _open

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("name", orf.NAMES)
def test_read_mel_gives_the_recorded_outside_features(ctx, name, layout):
    c = orf.case(name)
    s = _open(ctx, c)
    spec = c.reflected_spec(ctx)
    a, valid = c.raw_batch()
    L = a.shape[1]
    audio, v = s.read([0], [0], L, "ct", sample_rate=spec.sample_rate, channels=1)
    n = int(valid[0])
    assert v.tolist() == [n] and np.array_equal(audio.view(1, -1).cpu().numpy()[:, :n].view(np.uint32), a[:, :n].view(np.uint32))
    got, vf = s.read_mel([0], [0], c.n_frames, spec, layout=layout, length=L)
    torch.cuda.synchronize()
    spec.close()
    assert got.shape == ((1, spec.n_out, c.n_frames) if layout == "ct" else (1, c.n_frames, spec.n_out))
    assert vf.tolist() == c.valid_frames().tolist() == [(n + 80) // 160]
    oc.check(_btm(got, layout), c, "read_mel %s" % layout)
