"""Generator of the reference's listening demos (its hpss_audio/ set: the original signal and its _Harmonic and _Percussive versions
for speech, music and speech+music at several speech-to-music ratios), on the device: `silence.mix_signals` forms each mixture,
`Frontend.separate` splits it, scipy.io.wavfile writes <name>.wav, <name>_Harmonic.wav and <name>_Percussive.wav as 16-bit PCM.
WAV in, WAV out: no MP3 decoding or encoding.

    python tools/hpss_demo.py speech.wav music.wav --smr 20 15 10 5 0 -5 --out demos [--n-fft 400] [--stft-precision f32]

Names as the reference's: sp, mu, and sp+mu_<SMR>dB per ratio.  The mixtures all have the speech's length, so they go through
`separate` as one batch; speech and music go alone when their lengths differ from it."""
import argparse
import os
import sys

import numpy as np
import scipy.io.wavfile
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sm_hpss_mtl_amd import silence
from sm_hpss_mtl_amd.frontend import Frontend, FrontendConfig


def read_wav(path):
    """(fs, mono float32 in [-1, 1])"""
    fs, x = scipy.io.wavfile.read(path)
    if x.ndim == 2:
        x = x.mean(axis=1)
    if np.issubdtype(x.dtype, np.integer):
        x = x.astype(np.float64) / float(np.iinfo(x.dtype).max + 1) - (0.5 if x.dtype == np.uint8 else 0.0)
    return fs, np.ascontiguousarray(x, dtype=np.float32)


def to_int16(y):
    """float -> 16-bit PCM, rounded to nearest, clipped."""
    return np.clip(np.rint(np.asarray(y, np.float64) * 32767.0), -32768, 32767).astype(np.int16)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("speech")
    ap.add_argument("music")
    ap.add_argument("--smr", type=float, nargs="*", default=[20, 15, 10, 5, 0, -5], help="speech-to-music ratios in dB")
    ap.add_argument("--out", default=".")
    ap.add_argument("--n-fft", type=int, default=400)
    ap.add_argument("--win-length", type=int, default=400)
    ap.add_argument("--hop", type=int, default=160)
    ap.add_argument("--l-harm", type=int, default=21)
    ap.add_argument("--l-perc", type=int, default=11)
    ap.add_argument("--stft-precision", default="f32", choices=["f32", "f64"])
    args = ap.parse_args(argv)
    fs, sp = read_wav(args.speech)
    fs_mu, mu = read_wav(args.music)
    if fs != fs_mu:
        raise SystemExit("speech is sampled at %d Hz, music at %d Hz: resample one of them first" % (fs, fs_mu))
    fe = Frontend(FrontendConfig(n_fft=args.n_fft, win_length=args.win_length, hop=args.hop, l_harm=args.l_harm, l_perc=args.l_perc,
                                 stft_precision=args.stft_precision))
    sp_d, mu_d = torch.from_numpy(sp).cuda(), torch.from_numpy(mu).cuda()
    names, signals = ["sp", "mu"], [sp_d, mu_d]
    if args.smr:
        n = len(args.smr)
        mixes = silence.mix_signals(sp_d[None].expand(n, -1).contiguous(), mu_d[None].expand(n, -1).contiguous(),
                                    torch.tensor(args.smr, dtype=torch.float32))
        names += ["sp+mu_%gdB" % r for r in args.smr]
        signals += list(mixes)
    parts = fe.separate(signals)
    os.makedirs(args.out, exist_ok=True)
    written = []
    for name, x, yh, yp in zip(names, signals, parts["harmonic"], parts["percussive"]):
        for suffix, y in (("", x), ("_Harmonic", yh), ("_Percussive", yp)):
            path = os.path.join(args.out, name + suffix + ".wav")
            scipy.io.wavfile.write(path, fs, to_int16(y.cpu().numpy()))
            written.append(path)
    print("wrote %d files to %s" % (len(written), args.out))
    return written


if __name__ == "__main__":
    main()
