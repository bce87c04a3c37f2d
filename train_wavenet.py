"""Drop-in for the reference's train_wavenet.py: the teacher's training loop on one GPU (nsynth_wavenet_amd/train_cli.py).

    python train_wavenet.py --config config_jsons/wavenet_mol.json --train_path train.tfrecord --log_root logs --num_iters 200000
    python train_wavenet.py --train_path train.tfrecord --logdir logs/wavenet-<stamp> --num_iters 200000      # continue
"""
from nsynth_wavenet_amd import train_cli

if __name__ == '__main__':
    train_cli.main('teacher')
