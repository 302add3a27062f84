#!/usr/bin/env python3
"""Post-hoc temperature scaling of an existing checkpoint: fit T on the validation split, add the ``temperature``
key to the checkpoint in place (every other key is written back unchanged) and print one JSON line with T and the
NLL / ECE of the split before and after.

    python tools/calibrate.py --ckpt save/best.pth [the flags of main.py that describe the model and the data]

The forward is the one ``validate`` uses (``--val_img_stride``, ``--infer_window``, ``--tta_flips`` ... apply), the
fit makes ``--calibration_rounds`` passes (default 2), and ``--temperature`` sets the temperature of the "before"
numbers (default: the checkpoint's own, 1.0 for a checkpoint without one).  Predict mode and ``val_best`` then read the
temperature from the checkpoint.
"""
import argparse
import json
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from medical_segmentation_pytorch_amd.configs import MyConfig, load_parser
    from medical_segmentation_pytorch_amd.core import SegTrainer
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument('--ckpt', default=None, help='checkpoint to calibrate (default: <save_dir>/best.pth)')
    a, rest = ap.parse_known_args(argv)
    warnings.filterwarnings('ignore')
    config = load_parser(MyConfig().init_dependent_config(), rest)
    ckpt = a.ckpt or os.path.join(config.save_dir, 'best.pth')
    if not os.path.isfile(ckpt):
        sys.exit(f'calibrate: no checkpoint at {ckpt}')
    config.metrics = list(config.metrics) + [m for m in ('ece', 'nll') if m not in config.metrics]
    config.load_ckpt, config.use_tb = False, False
    trainer = SegTrainer(config)
    trainer.val_best(config, trainer.val_loader, ckpt_path=ckpt)
    before = trainer.val_history[-1]
    T = trainer.calibrate(config, trainer.val_loader, ckpt_path=ckpt)
    after = trainer.val_history[-1]
    out = {'tool': 'calibrate', 'ckpt': ckpt, 'T': T, 'T_before': before['calibration']['temperature'],
           'rounds': int(config.calibration_rounds), 'pixels': sum(after['calibration']['count']),
           'nll_before': before['nll'], 'nll_after': after['nll'], 'ece_before': before['ece'],
           'ece_after': after['ece'], config.metrics[0]: after[config.metrics[0]]}
    print(json.dumps(out), flush=True)
    return out


if __name__ == '__main__':
    main()
