"""train.py of the reference as a command:

    python -m ssd_amd.train --config config.json [--model_dir DIR] [--max_steps N] [--save_checkpoints_steps N]
                            [--eval_every_steps N] [--log_every N] [--seed S] [--no_eval]
                            [--save-summary-steps N] [--loss-histograms] [--gpus N] [--gpu-metric]

One JSON file of the reference drives everything (model_dir, train_dataset, val_dataset, pretrained_checkpoint and the model, loss,
input and optimizer keys).  A model_dir that holds a checkpoint resumes; otherwise the backbone is warm-started from
pretrained_checkpoint.  Every evaluation's dict is printed as one JSON line; the training log is model_dir/train_log.jsonl, and
TensorBoard reads model_dir/events.out.tfevents.* (scalars and the histograms of every variable and gradient, every
--save-summary-steps steps; 0: none; --loss-histograms adds the ten per-level top-20 % loss histograms of ssd.py:135-152 to each) and
model_dir/eval/.
--gpus N trains data-parallel on N GPUs of this node, one process each (Trainer's `group`: the config's batch_size is per GPU and
initial_learning_rate is used as given); train_dataset needs at least N shards.
"""


def main(argv=None):
    import argparse
    import json
    import os
    import sys
    from .trainer import EVAL_THROTTLE_SECS, SAVE_CHECKPOINTS_SECS, SAVE_SUMMARY_STEPS, Trainer
    ap = argparse.ArgumentParser(description="train.py's loop: train, checkpoint, evaluate the moving averages")
    ap.add_argument("--config", required=True, help="the reference's JSON config")
    ap.add_argument("--model_dir", default=None, help="default: the config's model_dir")
    ap.add_argument("--max_steps", type=int, default=None, help="default: the config's num_steps")
    ap.add_argument("--save_checkpoints_steps", type=int, default=None, help="default: every %d seconds" % SAVE_CHECKPOINTS_SECS)
    ap.add_argument("--eval_every_steps", type=int, default=None, help="default: every %d seconds" % EVAL_THROTTLE_SECS)
    ap.add_argument("--log_every", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save-summary-steps", "--save_summary_steps", dest="save_summary_steps", type=int, default=SAVE_SUMMARY_STEPS,
                    help="TensorBoard summaries every N steps, 0: none (default: %d)" % SAVE_SUMMARY_STEPS)
    ap.add_argument("--loss-histograms", "--loss_histograms", dest="loss_histograms", action="store_true",
                    help="with summaries on: also classification_losses_on_level_3..7 / localization_losses_on_level_3..7, the top "
                         "20 %% of every level's per-anchor losses (default: off)")
    ap.add_argument("--no_eval", action="store_true", help="train only")
    ap.add_argument("--gpus", type=int, default=1,
                    help="data-parallel training over N processes: N > 1 starts torch.distributed.run with N ranks as a child process "
                         "(rank r on device LOCAL_RANK %% device_count; RCCL only when every rank has a device of its own, else "
                         "gloo); inside such a launch the exchange runs, also at N = 1")
    ap.add_argument("--gpu-metric", "--gpu_metric", dest="gpu_metric", action="store_true",
                    help="every evaluation's AP on the training GPU (voc_match.VocEvaluator) instead of the host loop")
    a = ap.parse_args(argv)
    if a.gpus < 1:
        ap.error("--gpus must be >= 1")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        from .distributed import launch_local
        # nothing here has touched the GPU yet; the child runs this module again, once per rank
        sys.exit(launch_local(a.gpus, "ssd_amd.train", sys.argv[1:] if argv is None else list(argv)))

    def run(trainer, show):
        if a.no_eval:
            trainer.train(a.max_steps, a.save_checkpoints_steps, log_every=a.log_every, save_summary_steps=a.save_summary_steps,
                          loss_histograms=a.loss_histograms)
            return
        trainer.train_and_evaluate(a.max_steps, a.eval_every_steps, save_checkpoints_steps=a.save_checkpoints_steps,
                                   log_every=a.log_every, save_summary_steps=a.save_summary_steps, loss_histograms=a.loss_histograms,
                                   on_eval=(lambda res: print(json.dumps(res, sort_keys=True), flush=True)) if show else None)
    if "WORLD_SIZE" not in os.environ:
        run(Trainer(a.config, model_dir=a.model_dir, seed=a.seed, metric_device=0 if a.gpu_metric else None), True)
        return
    import torch.distributed as dist
    from .distributed import init_node_process_group
    if a.gpus != int(os.environ["WORLD_SIZE"]):
        raise SystemExit("--gpus (%d) != WORLD_SIZE (%s)" % (a.gpus, os.environ["WORLD_SIZE"]))
    device, _backend = init_node_process_group()
    try:
        run(Trainer(a.config, model_dir=a.model_dir, device=device, seed=a.seed, group=dist.group.WORLD,
                    metric_device=device if a.gpu_metric else None), dist.get_rank() == 0)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
