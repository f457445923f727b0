"""``python -m acousticswarms_speech_amd.mine_negatives DATASET [--sample_number N --start N]``: write every sample's
``challeng_sample.json``, the SRP-PHAT false positives the localization dataset draws its hard negatives from
(``train_data.mine_negatives``; the reference's datasets/generate_SRP_sample.py)."""
import argparse


def build_parser():
    p = argparse.ArgumentParser(prog="python -m acousticswarms_speech_amd.mine_negatives",
                                description="Mine SRP-PHAT false positives for a dataset of sample directories.")
    p.add_argument("dataset", type=str, help="Directory of sample directories 00000, 00001, ...")
    p.add_argument("--sample_number", type=int, default=1, help="Number of samples")
    p.add_argument("--start", type=int, default=0, help="Index of the first sample")
    p.add_argument("--device", type=str, default=None, help="Device of the pruner (default: the current one)")
    return p


def main(argv=None):
    from .train_data import mine_negatives
    args = build_parser().parse_args(argv)
    for d, (neg, pos) in mine_negatives(args.dataset, args.sample_number, args.start, device=args.device).items():
        print(f"{d}: {len(neg)} negative and {len(pos)} positive patches")


if __name__ == "__main__":
    main()
