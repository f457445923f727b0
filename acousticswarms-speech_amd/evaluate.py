"""The evaluation program, the counterpart of the reference's ``python sep/eval/eval_model.py``:

    python -m acousticswarms_speech_amd.evaluate DATASET --spot_experiment_dir D --sep_experiment_dir D
        [--results_folder F] [--spot_batch_size 128] [--batch N] [--metrics host|device] [--bss sdr|all]
        [--oracle irm,ibm]
        [--precision f16x3|f16x3_safe|f32] [--geometry host|device] [--use_cuda] [--cached_init]

Loads both networks with ``experiment.load_model_from_exp``, moves them to the GPU, builds the ``JointModel`` and runs
``evalkit.evaluate_dataset`` over every sample directory of DATASET; ends with the reference's closing lines
(sep/eval/eval_model.py:263-266).  The reference's flag names are kept.  Nothing runs at import."""
import argparse

PRECISIONS = ("f16x3", "f16x3_safe", "f32")


def oracle_names(text):
    """``--oracle irm,ibm`` -> ("irm", "ibm"); an unknown name is an argparse error."""
    from .evalkit import check_oracle
    try:
        return check_oracle(tuple(n.strip() for n in text.split(",") if n.strip()))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m acousticswarms_speech_amd.evaluate",
                                description="Evaluate the localisation + separation pipeline on a dataset directory.")
    p.add_argument("dataset", type=str, help="Path to the dataset directory")
    p.add_argument("--spot_experiment_dir", type=str, help="Experiment directory for spotforming submodel")
    p.add_argument("--sep_experiment_dir", type=str, help="Experiment directory for separation submodel")
    p.add_argument("--sr", type=float, default=48000, help="Sampling rate")
    p.add_argument("--n_mics", type=int, default=7, help="Number of microphones")
    p.add_argument("--use_cuda", dest="use_cuda", action="store_true",
                   help="Accepted for the reference's command lines; no effect: the networks always run on the GPU")
    p.add_argument("--spot_batch_size", dest="spot_batch_size", type=int, default=128,
                   help="Batch size for spotforming submodel")
    p.add_argument("--cached_init", action="store_true",
                   help="Accepted for the reference's command lines; no effect: the array geometry is rebuilt per sample")
    p.add_argument("--results_folder", type=str, default=None, help="Path to save results.json")
    p.add_argument("--batch", type=int, default=1,
                   help="Samples per batched call (evaluate_dataset(batch=)); 1: one sample at a time")
    p.add_argument("--metrics", choices=("host", "device"), default="host",
                   help="Where the BSS-eval SDR (and with --batch > 1 the SI-SDR matrices) are computed")
    p.add_argument("--bss", choices=("sdr", "all"), default="sdr",
                   help="BSS-eval fields of the record: the SDR alone, or SIR and SAR of both sets too")
    p.add_argument("--oracle", type=oracle_names, default=(),
                   help="Oracle mask baselines to score next to the output, comma-separated: irm, ibm")
    p.add_argument("--precision", choices=PRECISIONS, default="f32", help="Arithmetic of both networks")
    p.add_argument("--geometry", choices=("host", "device"), default="host", help="Where the array geometry is built")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.spot_experiment_dir or not args.sep_experiment_dir:
        raise SystemExit("--spot_experiment_dir and --sep_experiment_dir are both needed")
    from . import evalkit
    from .experiment import load_model_from_exp
    from .joint import JointModel
    device = "cuda:0"
    spot = load_model_from_exp(args.spot_experiment_dir, precision=args.precision, batch_size=args.spot_batch_size)
    sep = load_model_from_exp(args.sep_experiment_dir, precision=args.precision)
    model = JointModel(spot, sep, device=device, geometry=args.geometry).to(device)
    tot = evalkit.evaluate_dataset(model, args.dataset, args.results_folder, metrics=args.metrics, batch=args.batch,
                                   bss=args.bss, oracle=args.oracle)
    print("Overall tp: {}, fp: {}, fn: {}".format(tot["tp"], tot["fp"], tot["fn"]))
    print("Overall Precision: {} Recall: {}".format(tot["precision"], tot["recall"]))
    return tot


if __name__ == "__main__":
    main()
