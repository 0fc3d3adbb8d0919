/* sgw_view.h -- CPU ORACLE (TEST INFRASTRUCTURE ONLY): the agent-centric window shared by the multi-agent oracles.
 * Follows get_agent_perspective (safety_game_moma.py:1996-2101): the four visibilities, crop, pad with the character outside
 * the board, then np.rot90 by the observation direction. */
#ifndef SGW_VIEW_H_
#define SGW_VIEW_H_
#include <stdint.h>

#define SGW_VIEW_DEFAULT (-1)     /* given[0]: the window the oracle had before the radii could be given (`dflt` on every side) */
#define SGW_VIEW_NONE (-2)        /* given[0]: observation_radius=None, the whole board from wherever the agent stands */

/* given: an observation_radius argument in Directions order [LEFT, RIGHT, UP, DOWN] -> rad: [up, down, left, right].
 * None (:2003-2016): board size - 1 per axis, the larger of the two on every side where the window rotates. */
static inline void sgw_view_radii(const int32_t given[4], int dflt, int H, int W, int rotating, int rad[4]) {
  if (given[0] == SGW_VIEW_NONE) {
    int m = (H > W ? H : W) - 1;
    rad[0] = rad[1] = rotating ? m : H - 1; rad[2] = rad[3] = rotating ? m : W - 1;
  } else if (given[0] < 0) {
    rad[0] = rad[1] = rad[2] = rad[3] = dflt;
  } else {
    rad[0] = given[2]; rad[1] = given[3]; rad[2] = given[0]; rad[3] = given[1];
  }
}

static inline int sgw_view_square(const int rad[4]) { return rad[0] == rad[1] && rad[1] == rad[2] && rad[2] == rad[3]; }

/* turn: 0 none, 1 rot90 k=2 (facing DOWN), 2 rot90 k=-1 (facing LEFT), 3 rot90 k=1 (facing RIGHT); a turned window is square
 * (the callers refuse four different radii where the window rotates, as the engine does).  out: rows x cols, row-major. */
static inline void sgw_view_crop(const uint8_t* board, int H, int W, int row, int col, const int rad[4], int turn, uint8_t outside,
                                 uint8_t* out) {
  int rows = rad[0] + rad[1] + 1, cols = rad[2] + rad[3] + 1, n = rows;
  for (int i = 0; i < rows; ++i) for (int j = 0; j < cols; ++j) {
    int ci = i, cj = j;                                                  /* output cell (i, j) <- crop cell (ci, cj) */
    if (turn == 1) { ci = n - 1 - i; cj = n - 1 - j; }
    else if (turn == 2) { ci = n - 1 - j; cj = i; }                      /* clockwise: out[i][j] = in[n-1-j][i] */
    else if (turn == 3) { ci = j; cj = n - 1 - i; }                      /* counter-clockwise: out[i][j] = in[j][n-1-i] */
    int r = row - rad[0] + ci, c = col - rad[2] + cj;
    out[i * cols + j] = (r < 0 || r >= H || c < 0 || c >= W) ? outside : board[r * W + c];
  }
}
#endif
