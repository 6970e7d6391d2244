#!/usr/bin/env python3
"""Generate tests/golden/rect.npz by running the REFERENCE's generators on inputs that are not square: the eval-mode outputs of
its Autoencoder and its VariationalAutoencoder (with an injected eps; also mu and logvar) for one 48x80 and one 32x48 input under
`synth.state_dict_like` parameters.  Only the outputs are stored: inputs, eps and parameters are rebuilt from the seed by the test (synth).

Runs only where the reference is (it never travels); the file it writes is committed.

    python tests/golden/make_golden_rect.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import EpsInjector, import_reference, load_synth_params, synth  # noqa: E402
from cases import SEED, STEP_BIAS_STD  # noqa: E402

SIZES = ((48, 80), (32, 48))
LATENT = 64


def main():
    torch.set_num_threads(8)
    N, _ = import_reference()
    out = {}
    ae = N.Autoencoder()
    load_synth_params(ae, SEED, STEP_BIAS_STD, prefix="rect_ae.")
    ae.eval()
    vae = N.VariationalAutoencoder(latent_dim=LATENT)
    load_synth_params(vae, SEED, STEP_BIAS_STD, prefix="rect_vae.")
    vae.eval()
    for h, w in SIZES:
        key = f"{h}x{w}"
        x = synth.uniform((1, 3, h, w), SEED, f"rect/x/{key}")
        eps = synth.normal((1, LATENT, h // 16, w // 16), SEED, f"rect/eps/{key}")
        with torch.no_grad():
            y = ae(torch.from_numpy(x))
            with EpsInjector([eps]):
                gx, mu, logvar = vae(torch.from_numpy(x))
        out[f"{key}/ae"], out[f"{key}/vae"] = y.numpy(), gx.numpy()
        out[f"{key}/mu"], out[f"{key}/logvar"] = mu.numpy(), logvar.numpy()
        print(key, "ae", tuple(y.shape), "vae", tuple(gx.shape), "mu", tuple(mu.shape))
    path = os.path.join(HERE, "rect.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
