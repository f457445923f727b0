"""Function-preserving rescalings of the two networks' weights, shared by test_rescaling_oracle_host.py and
test_gpu_safe_precision.py.

ReLU is positively homogeneous, so for s > 0
    linear2(relu(linear1(x)))                       with linear1.{weight,bias} * s,      linear2.weight / s
    output_decoder(relu(mask_encoder(x)) * bypass)  with mask_encoder.{weight,bias} * s, output_decoder.weight / s
compute what they computed before while the feed-forward hidden layer and the masked latent grow by s.  With s a
power of two every product and sum scales exactly (short of overflow and underflow), so the fp32 result is the same
bit for bit whatever the order of the additions.  The Conformer's feed-forward modules use Swish, which is not
homogeneous, and stay as they are; so do the V rows of in_proj_weight (the split weights carry one power-of-two
pre-scale per tensor: scaling a third of the rows would push the rest into fp16 subnormals)."""
import numpy as np

S = 2.0 ** 20


def _scaled(sd, up, down, s):
    out = dict(sd)
    for k in up:
        out[k] = (np.asarray(sd[k], dtype=np.float32) * np.float32(s)).astype(np.float32)
    for k in down:
        out[k] = (np.asarray(sd[k], dtype=np.float32) / np.float32(s)).astype(np.float32)
    return out


def rescale_spot(sd, cfg, s=S):
    """both transformer layers' feed-forward pair and the mask path"""
    up, down = ["mask_encoder.weight", "mask_encoder.bias"], ["output_decoder.weight"]
    for l in range(cfg.num_transformer_layers):
        p = f"bottleneck.transf.layers.{l}"
        up += [p + ".linear1.weight", p + ".linear1.bias"]
        down += [p + ".linear2.weight"]
    return _scaled(sd, up, down, s)


def rescale_sep(sd, cfg, s=S):
    """every inter-speaker layer's feed-forward pair and the mask path"""
    up, down = ["mask_encoder.weight", "mask_encoder.bias"], ["output_decoder.weight"]
    for l in range(cfg.bottleneck_layers):
        p = f"bottleneck.module_list.{l}.inter.layers.0"
        up += [p + ".linear1.weight", p + ".linear1.bias"]
        down += [p + ".linear2.weight"]
    return _scaled(sd, up, down, s)


SPOT_OFFSETS = [np.array([0, 0, 0, 0, 0, 0]), np.array([3, -5, 8, -13, 21, -34])]
