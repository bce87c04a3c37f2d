"""Drop-in for the reference's train_parallel_wavenet.py: the student's distillation loop on one GPU under a trained
teacher (nsynth_wavenet_amd/train_cli.py).

    python train_parallel_wavenet.py --config config_jsons/parallel_wavenet.json --train_path train.tfrecord \
        --teacher_dir logs/wavenet-<stamp> --log_root logs --num_iters 400000
"""
from nsynth_wavenet_amd import train_cli

if __name__ == '__main__':
    train_cli.main('student')
