"""train.py of the reference as a command:

    python -m ssd_amd.train --config config.json [--model_dir DIR] [--max_steps N] [--save_checkpoints_steps N]
                            [--eval_every_steps N] [--log_every N] [--seed S] [--no_eval]
                            [--save-summary-steps N]

One JSON file of the reference drives everything (model_dir, train_dataset, val_dataset, pretrained_checkpoint and the model, loss,
input and optimizer keys).  A model_dir that holds a checkpoint resumes; otherwise the backbone is warm-started from
pretrained_checkpoint.  Every evaluation's dict is printed as one JSON line; the training log is model_dir/train_log.jsonl, and
TensorBoard reads model_dir/events.out.tfevents.* (scalars and the histograms of every variable and gradient, every
--save-summary-steps steps; 0: none) and model_dir/eval/.
"""


def main(argv=None):
    import argparse
    import json
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
    ap.add_argument("--no_eval", action="store_true", help="train only")
    a = ap.parse_args(argv)
    trainer = Trainer(a.config, model_dir=a.model_dir, seed=a.seed)
    if a.no_eval:
        trainer.train(a.max_steps, a.save_checkpoints_steps, log_every=a.log_every, save_summary_steps=a.save_summary_steps)
        return
    trainer.train_and_evaluate(a.max_steps, a.eval_every_steps, save_checkpoints_steps=a.save_checkpoints_steps, log_every=a.log_every,
                               save_summary_steps=a.save_summary_steps, on_eval=lambda res: print(json.dumps(res, sort_keys=True), flush=True))


if __name__ == "__main__":
    main()
