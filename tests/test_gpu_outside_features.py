"""The feature front ends on the GPU against an implementation this project did not write: the user's whole path -- bytes of FLAC
in, "Whisper's input", "Kaldi's fbank" or "Kaldi's MFCC" out -- held to the recorded answers of transformers.audio_utils,
WhisperFeatureExtractor and scipy.fft.dct (tests/golden/features, written by tools/make_feature_goldens.py; the rules and the bounds
are outside_cases.py's).  Each case's PCM becomes a FLAC stream of 256-sample blocks with a short last frame, is
opened with open_streams and read with read_mel in both layouts; the two Whisper streams, one mono and short, one stereo and a full
second, share one set and one call; kaldi16 is also read from sample 777; and for each front end one raw Context.mel_windows call
on the fixture's audio writes a guarded slice.  The file reads the fixtures only."""
import numpy as np
import pytest
import torch

import claxon_amd as cx
import md5_cases as mc
import outside_cases as oc
import synth
from gpu_guarded import device_out, written

pytestmark = pytest.mark.gpu
BS = 256


@pytest.fixture(scope="module")
def ctx():
    return cx.Context(0, wait_s=120)


def _flac(pcm, rate):
    """A 16-bit FLAC stream of the int16 samples pcm [T, C] at `rate`: blocks of 256 and one short last frame, so that windows cross
    frame boundaries; fixed and LPC subframes and, in stereo, the four channel assignments in turn."""
    T, ch = pcm.shape
    n, last = (T - 1) // BS, T - BS * ((T - 1) // BS)
    assert 0 < last <= BS and n >= 1

    def frames(x, bs, number0):
        k = x.shape[0] // bs
        fp = [synth.FrameParams() for _ in range(k)]
        po = max(p for p in range(4) if bs % (1 << p) == 0 and (bs >> p) >= 32 or p == 0)
        for i, f in enumerate(fp):
            f.number = number0 + i
            f.channel_assignment = (i % 4) if ch == 2 else 0
            for c in range(ch):
                f.sf[c] = synth.sf(synth.SF_LPC if (i + c) % 3 else synth.SF_FIXED, order=8 if (i + c) % 3 else 2, precision=12, partition_order=po)
        return synth.encode_frames("outside", np.ascontiguousarray(x.reshape(k, bs, ch).transpose(0, 2, 1)).astype(np.int32), ch, bs, 16, fp,
                                   sample_rate=rate)

    w = synth.concat("outside", [frames(pcm[:n * BS], BS, 0), frames(pcm[n * BS:], last, n)])
    vals = pcm.astype(np.int64).reshape(-1)
    si = bytearray(mc.streaminfo(BS, ch, 16, T, mc.ref_md5(vals, 16)))
    si[18:22] = ((rate << 12) | ((ch - 1) << 9) | (15 << 4) | (T >> 32)).to_bytes(4, "big")       # (the rate: md5_cases writes 44.1 kHz)
    return bytes(si) + b"".join(w.arena[int(w.offs[i]):int(w.offs[i] + w.lens[i])].tobytes() for i in range(w.n))


_SETS = {}


def _open(ctx, c):
    """The case's streams as one resident set, opened once; their decode is the fixture's PCM."""
    if c.name not in _SETS:
        s = cx.open_streams(ctx, [_flac(p, c.p["sample_rate"]) for p in c.streams])
        assert s.problems == [None] * len(c.streams) and s.sample_rates == [c.p["sample_rate"]] * len(c.streams)
        assert s.channels == [p.shape[1] for p in c.streams] and [int(n) for n in s.lengths] == [p.shape[0] for p in c.streams]
        _SETS[c.name] = s
    return _SETS[c.name]


def _btm(t, layout):
    o = t.cpu().numpy()
    return o.transpose(0, 2, 1) if layout == "ct" else o


@pytest.mark.parametrize("layout", ("ct", "tc"))
@pytest.mark.parametrize("name", oc.NAMES)
def test_read_mel_gives_the_recorded_outside_features(ctx, name, layout):
    """FLAC in, features out, one read_mel call over all the case's windows: the audio that reaches the kernel is the fixture's
    (read(..., channels=1) of the same windows, bit for bit), valid_frames follows the spec's rule, and every cell lies in the
    interval around the outside value, with the vacuity cap; a frame past valid_frames is exactly 0 -- in the Whisper cases what
    the extractor gives for its own zero padding."""
    c = oc.case(name)
    s = _open(ctx, c)
    spec = c.spec(ctx)
    sid, st = [w[0] for w in c.windows], [w[1] for w in c.windows]
    a, valid = c.batch()
    audio, v = s.read(sid, st, a.shape[1], "ct", sample_rate=spec.sample_rate, channels=1)
    assert np.array_equal(audio.view(len(sid), -1).cpu().numpy().view(np.uint32), a.view(np.uint32)) and v.tolist() == valid.tolist()
    got, vf = s.read_mel(sid, st, c.n_frames, spec, layout=layout)
    torch.cuda.synchronize()
    spec.close()
    assert got.shape == ((len(sid), spec.n_out, c.n_frames) if layout == "ct" else (len(sid), c.n_frames, spec.n_out))
    assert vf.tolist() == c.valid_frames().tolist()
    oc.check(_btm(got, layout), c, "read_mel %s" % layout)


@pytest.mark.parametrize("name", ("htk_ln", "whisper80", "kaldi16", "mfcc16_energy"))
def test_raw_mel_windows_on_the_fixture_audio(ctx, name):
    """One front end each -- clx_k_mel, clx_k_mel_c with clx_k_mel_range, clx_k_mel_f, clx_k_mel_q -- without the decode in
    between: Context.mel_windows on the fixture's batch into a guarded slice, held as the simulator's output is."""
    c = oc.case(name)
    spec = c.spec(ctx)
    a, valid = c.batch()
    B, T = a.shape[0], c.n_frames
    n = B * spec.n_out * T
    for layout in ("ct", "tc"):
        flat, out = device_out(n, offset_words=1)
        dev = torch.from_numpy(a).to("cuda:0")
        torch.cuda.synchronize()                             # (the fill first: on torch's default stream the launch goes to the context's own)
        ctx.mel_windows(spec, dev, valid, T, cx._LAYOUTS[layout], out.view((B, spec.n_out, T) if layout == "ct" else (B, T, spec.n_out)))
        torch.cuda.synchronize()
        o = written(flat, n, (name, layout), offset_words=1).view(np.float32)
        oc.check(o.reshape(B, spec.n_out, T).transpose(0, 2, 1) if layout == "ct" else o.reshape(B, T, spec.n_out), c, "mel_windows %s" % layout)
    spec.close()
