"""Global planner: occupancy map -> enlarged obstacles -> shortest 8-connected path -> waypoint follower.

Mirrors ``robotmpcs.global_planner`` (``gridmap.OccupancyGridMap``, ``a_star.a_star``, ``globalPlanner.GlobalPlanner``:
same module, class and method names, so that a port of ``examples/boxer_example_global.py`` changes only its imports)
and adds the batched, device-resident fleet API (``plan_batch``, ``RouteFollower``, ``replan``, ``shelf_map``) and the
fleet's conflict-free timed routes (``TimedRoutes``, ``TimedFollower``) and the pairing of robots with goals at the least
sum of route costs (``GoalAssigner``) and tours of several goals per robot with a follower that stops at them
(``TourPlanner``, ``TourFollower``; ``rmpc_tours_device`` / ``rmpc_follow_tour_device``, include/rmpc_tours.h) and the two
together, timed tours through every robot's stops (``TimedTours``, ``TimedTourFollower``; include/rmpc_timed_tours.h), re-planned
for part of the fleet while it is under way (``LifelongTours``, ``rebase``; include/rmpc_timed_replan.h), and any-angle
routes: line of sight on the grid, routes pulled tight by it and a follower that looks ahead (``visible``, ``shorten_routes``,
``route_lengths``, ``VisibleFollower``; include/rmpc_any_angle.h), and routes that know about each other: congestion and
contraflow costs from a table of the fleet's flow (``TrafficRoutes``; include/rmpc_traffic.h), and timed routes with the
least sum of arrivals, or a lower bound on it, by conflict-based search (``OptimalTimedRoutes``; include/rmpc_cbs.h),
or plans the whole fleet within a stated factor of that sum by focal search (``BoundedTimedRoutes``; include/rmpc_ecbs.h).  The work is done
by the ``rmpc_grid_*_device`` / ``rmpc_follow_path_device`` / ``rmpc_timed_*_device`` kernels (include/rmpc.h); there is no CPU path.  Importing
the package needs no GPU.
"""
from .gridmap import OccupancyGridMap
from .a_star import a_star
from .globalPlanner import FREE, OCC, GlobalPlanner, png_values
from .batch import RouteFollower, cell_xy, cells_from_positions, pick_routes, plan_batch, replan, shelf_map, store_routes
from .dispatch import GoalAssigner
from .timed import TimedFollower, TimedRoutes, pick_spaced_routes, priority_orders
from .tours import TourFollower, TourPlanner
from .timed_tours import TimedTourFollower, TimedTours, pick_spaced_tours
from .lifelong import LifelongTours, rebase
from .any_angle import VisibleFollower, route_lengths, shorten_routes, visible
from .traffic import TrafficRoutes
from .optimal import BoundedTimedRoutes, OptimalTimedRoutes

__all__ = ["BoundedTimedRoutes", "FREE", "OCC", "OccupancyGridMap", "a_star", "GlobalPlanner", "GoalAssigner", "LifelongTours", "OptimalTimedRoutes", "RouteFollower", "TimedFollower", "TimedRoutes", "TimedTourFollower", "TimedTours", "TourFollower", "TourPlanner", "TrafficRoutes", "VisibleFollower", "cell_xy", "cells_from_positions",
           "pick_routes", "pick_spaced_routes", "pick_spaced_tours", "plan_batch", "png_values", "priority_orders", "rebase", "replan", "route_lengths", "shelf_map", "shorten_routes", "store_routes", "visible"]
