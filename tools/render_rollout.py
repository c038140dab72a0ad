#!/usr/bin/env python3
"""Frames of k test episodes of a trained tracker: python tools/render_rollout.py --env_config E --agent_config A --model_file M
--render_dir DIR [--episodes k] [--render_envs 0,1] [--render_size 640x360] [--num_envs n] [--gif]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parc_amd import render
from parc_amd.envs import base_env, env_builder
from parc_amd.learning import agent_builder
from parc_amd.util import arg_parser


def main(argv):
    args = arg_parser.ArgParser()
    args.load_args(argv[1:])
    device = args.parse_string("device", "cuda:0")
    ids = [int(x) for x in args.parse_string("render_envs", "0").split(",")]
    env = env_builder.build_env(args.parse_string("env_config"), args.parse_int("num_envs", max(ids) + 1), device, False)
    agent = agent_builder.build_agent(args.parse_string("agent_config"), env, device)
    agent.load(args.parse_string("model_file"))
    env.set_mode(base_env.EnvMode.TEST)
    w, h = render.parse_size(args.parse_string("render_size", "640x360"))
    writer = render.FrameWriter(args.parse_string("render_dir"), env_ids=ids, gif=args.has_key("gif"))
    env.set_renderer(render.Renderer(env, w, h, ids), writer)
    res = agent.test_model(num_episodes=args.parse_int("episodes", 1))
    writer.close()
    print("Mean Return: {}  Episodes: {}  frames: {}".format(res["mean_return"], res["num_eps"], len(writer.paths)))


if __name__ == "__main__":
    main(sys.argv)
