"""``python -m acousticswarms_speech_amd.validate EXPERIMENT_DIR [--checkpoint N | --all] [--backend device|host]``: the
validation loss of an experiment's checkpoints, computed as the reference's trainer does (``train_data.validate``) on
the test set its ``description.json`` names (``test_set_params``) -- the number ``load_model_from_exp(mode="best")``
ranks checkpoints by."""
import argparse
import glob
import json
import os


def build_parser():
    p = argparse.ArgumentParser(prog="python -m acousticswarms_speech_amd.validate",
                                description="Validation loss of an experiment's checkpoints.")
    p.add_argument("experiment_dir", type=str)
    which = p.add_mutually_exclusive_group()
    which.add_argument("--checkpoint", type=int, default=None, help="Epoch of the checkpoint (default: the last)")
    which.add_argument("--all", action="store_true", help="One line per checkpoint, and the best")
    p.add_argument("--backend", choices=("device", "host"), default="device", help="Where the batches are made")
    p.add_argument("--test_dir", type=str, default=None, help="Override test_set_params.input_dir")
    p.add_argument("--batch_size", type=int, default=None, help="Override training_params.batch_size")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--precision", type=str, default="f32")
    return p


def checkpoints(exp_dir, desc):
    """-> (experiment name, {epoch: path}) as ``load_model_from_exp`` finds them."""
    name = desc["experiment_name"] if "experiment_name" in desc else os.path.basename(exp_dir.strip("/"))
    ckpt_dir = name if "experiment_name" in desc else "checkpoints"
    paths = glob.glob(os.path.join(exp_dir, ckpt_dir, f"{name}_*.pt"))
    return name, {int(p[p.rfind("_") + 1:-len(".pt")]): p for p in paths}


def main(argv=None):
    from . import train_data
    from .experiment import _safe_load, load_model_from_exp
    args = build_parser().parse_args(argv)
    with open(os.path.join(args.experiment_dir, "description.json"), "rb") as f:
        desc = json.load(f)
    _name, ckpts = checkpoints(args.experiment_dir, desc)
    if not ckpts:
        raise SystemExit(f"{args.experiment_dir}: no checkpoint found")
    epochs = sorted(ckpts) if args.all else [max(ckpts) if args.checkpoint is None else args.checkpoint]
    cls = train_data.LocalizationDataset if desc["model_name"] == "SpeakerLocalization" else train_data.SeparationDataset
    set_params = dict(desc.get("test_set_params", {}))          # holds input_dir, as the reference's trainer expects
    if "sr" in desc:
        set_params["sr"] = desc["sr"]
    if args.test_dir:
        set_params["input_dir"] = args.test_dir
    dataset = cls(dataset_type="test", **set_params)
    params = desc.get("training_params", {})
    model = load_model_from_exp(args.experiment_dir, mode="new", precision=args.precision)
    results = {}
    for epoch in epochs:
        if epoch not in ckpts:
            raise SystemExit(f"no checkpoint of epoch {epoch}; there are {sorted(ckpts)}")
        model.load_state_dict(_safe_load(ckpts[epoch]), strict=True)
        res = train_data.validate(model.to(args.device), dataset, loss=params.get("loss", "snr"),
                                  batch_size=args.batch_size or params.get("batch_size", 8), backend=args.backend)
        results[epoch] = res["loss"]
        gain = [o - i for i, o in zip(res["input_si_sdr"], res["output_si_sdr"])]
        print(f"checkpoint {epoch}: loss {res['loss']:.6f}, SI-SDR improvement "
              f"{sum(gain) / len(gain) if gain else float('nan'):.3f} dB over {len(gain)} positive rows")
    if args.all:
        best = min(results, key=results.get)
        print(f"best: checkpoint {best} (loss {results[best]:.6f})")
    return results


if __name__ == "__main__":
    main()
