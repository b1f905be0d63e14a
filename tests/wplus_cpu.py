"""W+ restatement of the CPU oracle (TEST INFRASTRUCTURE): oracle.latent_aug_ref.LatentAugRef with the W+ contract's replacements.
The contract replaces three methods of the reference's LatentAug: broadcasting(latent) becomes the identity for a [b, num_ws, w_dim]
latent, hard_aug(w, w_tilde) returns w_tilde and smooth_aug(w, w_tilde) blends alpha * w_tilde + (1 - alpha) * w row by row.  The
oracle writes its gate inline as broadcasting(w_opt) / broadcasting(alpha * w_opt + (1 - alpha) * w), so replacing broadcasting() here
is all three.  Adam, the criteria, the crops and the loss signs are the oracle's.  Pinned to a run of the reference with the same
replacements (tests/golden/wplus_loop.npz, made by tests/golden/make_golden_wplus.py)."""
import torch

from oracle import latent_aug_ref as lar


class LatentAugRefWPlus(lar.LatentAugRef):
    def broadcasting(self, w):
        assert w.shape[1] == self.num_ws, 'W+ latents carry one row per style slot'
        return w


def run_f64(ref_kw, G, D, W, X, fea, feature_net, w0, crop_pos):
    """The same W+ loop in float64 (tolerance anchor): modconv unfused, networks and banks in float64 for the run."""
    from oracle import sg2_networks as nets
    nets.COMPUTE_DTYPE = torch.float64
    mods = [m for m in (G, D, feature_net) if m is not None]
    try:
        for m in mods:
            m.double()
        dbl = (lambda t: t.double() if t is not None else None)
        ref = LatentAugRefWPlus(G, D, W=dbl(W), X=dbl(X), fea=[f.double() for f in fea] if fea is not None else None,
                                feature_net=feature_net, dtype=torch.float64, fused_modconv=False, **ref_kw)
        img, w_aug = ref.forward(w0, crop_pos=crop_pos, record=True)
        return img, w_aug, ref.trace
    finally:
        nets.COMPUTE_DTYPE = torch.float32
        for m in mods:
            m.float()
